// lbs_leaves.h -- the per-vertex device code of the skinning kernels: vector types, cache-policy loads / stores, the matrix product and
// the bone palette column, palette staging into the packed-math LDS layout (with the affine test, the workgroup flag and the unit
// ticket), skin_vertex (the reference's operation order, see lbs_kernels.hip's head) and the vertex streams as buffer resources.
// Shared by lbs_kernels.hip (every skinning kernel) and anim_kernels.hip (the pose kernels' palettes, the one-launch frame that goes on
// to the vertices): ONE definition, so a vertex skinned inside a pose launch has the bits of one skinned by lbs_skin.
#pragma once
#include "fyx_internal.h"

namespace fyx {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <bool NT, typename T>
__device__ __forceinline__ T ldg(const T* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT, typename T>
__device__ __forceinline__ void stg(T* p, T v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

template <bool NT>
__device__ __forceinline__ void ld3(const float* p, float& x, float& y, float& z) {
    x = ldg<NT>(p); y = ldg<NT>(p + 1); z = ldg<NT>(p + 2);
}
template <bool NT>
__device__ __forceinline__ void st3(float* p, float x, float y, float z) {
    stg<NT>(p, x); stg<NT>(p + 1, y); stg<NT>(p + 2, z);
}

// nalgebra's Matrix4 * Matrix4, one element: a = row i of the left matrix, b = column j of the right one, summed as the
// k-ascending axpy chain y = a0*b0; y = a1*b1 + y; ...  Every product of two matrices on the device (the hierarchy's walks,
// the palettes global * inv_bind) is this chain.
__device__ __forceinline__ float mat4_elem(f32x4 a, f32x4 b) {
    float y = a.x * b.x;
    y = a.y * b.y + y;
    y = a.z * b.z + y;
    y = a.w * b.w + y;
    return y;
}

// Column c of bone_matrices[b] = global(node) * inv_bind(node) (scene/mesh/mod.rs:781-793): g = the node's four global
// columns, ib = column c of its inverse bind matrix.  An invalid bone handle (node < 0) yields the identity's column.
__device__ __forceinline__ f32x4 bone_palette_column(const f32x4* g, f32x4 ib, int32_t node, uint32_t c) {
    if (node < 0) return f32x4{c == 0 ? 1.0f : 0.0f, c == 1 ? 1.0f : 0.0f, c == 2 ? 1.0f : 0.0f, c == 3 ? 1.0f : 0.0f};
    const f32x4* a = g + (size_t)node * 4;
    const f32x4 a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
    return f32x4{mat4_elem(f32x4{a0.x, a1.x, a2.x, a3.x}, ib), mat4_elem(f32x4{a0.y, a1.y, a2.y, a3.y}, ib),
                 mat4_elem(f32x4{a0.z, a1.z, a2.z, a3.z}, ib), mat4_elem(f32x4{a0.w, a1.w, a2.w, a3.w}, ib)};
}

// ---------------------------------------------------------------------------------------
// Palette staging: global column-major mat4 -> three float4 per bone in LDS, arranged for
// PACKED f32 math (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 work on register pairs and can
// broadcast either half of a pair):
//     A = (m00, m10, m01, m11)   B = (m02, m12, t0, t1)   C = (m20, m21, m22, t2)
// so the x and y rows of a matrix sit side by side in a 64-bit register pair
//   (pos.x, pos.y) = ((A.lo*px + A.hi*py) + B.lo*pz) + B.hi           3 pk_mul + 3 pk_add
// while a single coefficient m_rk is the lo or hi half of one of those pairs, so normal and
// tangent are transformed together as the pair (n_r, t_r) = (m_r0*(nx,tx) + m_r1*(ny,ty)) +
// m_r2*(nz,tz) with the coefficient broadcast by op_sel -- no register shuffling.  Every output
// component keeps exactly the reference's operation order (each pk instruction rounds its two
// lanes independently), so the packed EXACT path stays bit-identical to the CPU loop while
// issuing ~half the VALU instructions of the scalar form.
// row3[b] = (m30, m31, m32, m33) is only read by the projective path.
// Returns (per thread) whether any staged matrix is projective.
// ---------------------------------------------------------------------------------------
struct PaletteRegs {
    f32x4 c0, c1, c2, c3;
};

// Issue the global loads of this thread's bone (n_bones <= 256 <= BLOCK: at most one bone each).
__device__ __forceinline__ PaletteRegs palette_fetch(const float* __restrict__ pal, uint32_t n_bones,
                                                     int tid) {
    // unconditional (clamped) so that no branch sits between these loads, the vertex loads that
    // follow and the LDS commit: the compiler's vmcnt bookkeeping stays exact only in straight-line code
    const uint32_t b = (uint32_t)tid < n_bones ? (uint32_t)tid : n_bones - 1;
    const f32x4* m = reinterpret_cast<const f32x4*>(pal + (size_t)b * 16);
    PaletteRegs r;
    r.c0 = m[0]; r.c1 = m[1]; r.c2 = m[2]; r.c3 = m[3];
    return r;
}

// The affine test of a matrix's last row (m30, m31, m32, m33) = (0, 0, 0, 1): one column's entry w = m3c, and the whole row.
__device__ __forceinline__ bool column_projective(float w, uint32_t c) { return w != (c == 3 ? 1.0f : 0.0f); }
__device__ __forceinline__ bool row3_projective(f32x4 w) { return !(w.x == 0.0f && w.y == 0.0f && w.z == 0.0f && w.w == 1.0f); }

// Write column c = (m0c, m1c, m2c, m3c) of bone b into the packed-math layout: (x, y) is one 8-byte store, z and w one 4-byte
// store each.  True if the column breaks the affine last row.
__device__ __forceinline__ bool commit_column(f32x4* rows, f32x4* row3, uint32_t b, uint32_t c, f32x4 col) {
    float* r = reinterpret_cast<float*>(rows + b * 3);
    *reinterpret_cast<f32x2*>(r + 2 * c) = f32x2{col.x, col.y};
    r[8 + c] = col.z;
    reinterpret_cast<float*>(row3 + b)[c] = col.w;
    return column_projective(col.w, c);
}

// Write a whole bone into the packed-math layout with whole-row stores; true if that matrix is projective.
__device__ __forceinline__ bool commit_bone(const PaletteRegs& r, f32x4* rows, f32x4* row3, uint32_t b) {
    rows[b * 3 + 0] = f32x4{r.c0.x, r.c0.y, r.c1.x, r.c1.y};
    rows[b * 3 + 1] = f32x4{r.c2.x, r.c2.y, r.c3.x, r.c3.y};
    rows[b * 3 + 2] = f32x4{r.c0.z, r.c1.z, r.c2.z, r.c3.z};
    const f32x4 w = {r.c0.w, r.c1.w, r.c2.w, r.c3.w};
    row3[b] = w;
    return row3_projective(w);
}

// Write the fetched bone to LDS; true if that matrix is projective.
__device__ __forceinline__ bool palette_commit(const PaletteRegs& r, uint32_t n_bones, f32x4* rows,
                                               f32x4* row3, int tid) {
    if ((uint32_t)tid >= n_bones) return false;
    return commit_bone(r, rows, row3, tid);
}

// Whole-palette staging by a workgroup of any size (AABB kernel).
__device__ __forceinline__ bool stage_palette(const float* __restrict__ pal, uint32_t n_bones,
                                              f32x4* rows, f32x4* row3, int tid, int nthreads) {
    bool projective = false;
    for (uint32_t b = tid; b < n_bones; b += nthreads) {
        const f32x4* m = reinterpret_cast<const f32x4*>(pal + (size_t)b * 16);
        projective |= commit_bone(PaletteRegs{m[0], m[1], m[2], m[3]}, rows, row3, b);
    }
    return projective;
}

// The dyn kernels' palette staging (n_bones <= 256): every thread of a BLOCK-thread workgroup fetches 1024 / BLOCK 16-byte
// columns, the wave's FIRST vector-memory instruction; column c of bone b is piece 4 b + c, and a wave fetches 64 consecutive
// pieces (16 bones, one dense 1 KB request).  WHICH lane takes which piece of those 64 is chosen for the LDS commit: the 16
// lanes one ds_write_b64 serves together take the four columns of bones {0, 2, 4, 6} (or {1, 3, 5, 7}) of an octet, whose
// 8-dword (x, y) windows at the 48-byte row stride start at dwords 0 / 24 / 48 / 72 = banks 0 / 24 / 16 / 8: the four windows
// tile all 32 banks.  (With lanes in piece order the group was bones {0, 1, 2, 3}: windows at banks 0 / 12 / 24 / 4, the fourth
// on top of the first -- SQ_LDS_BANK_CONFLICT 65 536 cycles per launch in round 2.)  The 32 lanes of a 4-byte store (z, w)
// cover a whole octet of bones: dwords 12 b + 8 + c, all banks.
// EMPTY_OK: the palette may have no bone at all (a batch segment), so no column is fetched.
template <int BLOCK, bool EMPTY_OK = false>
struct PaletteColumns {
    static constexpr int kPieces = 1024 / BLOCK;
    f32x4 col[kPieces];

    __device__ __forceinline__ static uint32_t first_piece(uint32_t tid) {
        const uint32_t lane = tid & 63, grp16 = lane >> 4, in16 = lane & 15;
        return (tid & ~63u) + 4 * (8 * (grp16 >> 1) + 2 * (in16 >> 2) + (grp16 & 1)) + (in16 & 3);
    }
    __device__ __forceinline__ void fetch(const float* __restrict__ pal, uint32_t n_bones, uint32_t piece0) {
        const uint32_t n_pieces = n_bones * 4;
#pragma unroll
        for (int i = 0; i < kPieces; ++i) {
            const uint32_t piece = piece0 + (uint32_t)i * BLOCK;
            const f32x4* p = reinterpret_cast<const f32x4*>(pal);
            if constexpr (EMPTY_OK) col[i] = n_pieces ? p[piece < n_pieces ? piece : n_pieces - 1] : f32x4{0.f, 0.f, 0.f, 0.f};
            else col[i] = p[piece < n_pieces ? piece : n_pieces - 1];
        }
    }
    // true if a column this thread staged breaks the affine last row
    __device__ __forceinline__ bool commit(uint32_t n_bones, uint32_t piece0, f32x4* rows, f32x4* row3) const {
        const uint32_t n_pieces = n_bones * 4;
        bool pj = false;
#pragma unroll
        for (int i = 0; i < kPieces; ++i) {
            const uint32_t piece = piece0 + (uint32_t)i * BLOCK;
            if (piece < n_pieces) pj |= commit_column(rows, row3, piece >> 2, piece & 3, col[i]);
        }
        return pj;
    }
};

// Workgroup OR of the threads' projective flags, one LDS word per wave: publish the wave's bit, and after a barrier read the
// workgroup's (block_projective: both around the barrier the palette staging needs anyway).
__device__ __forceinline__ void publish_projective(bool pj, uint32_t* wave_flag, uint32_t lane, uint32_t wave) {
    const bool wave_pj = __any(pj) != 0;
    if (lane == 0) wave_flag[wave] = wave_pj ? 1u : 0u;
}
template <uint32_t WPB>
__device__ __forceinline__ bool read_projective(const uint32_t* wave_flag) {
    bool projective = false;
#pragma unroll
    for (uint32_t wv = 0; wv < WPB; ++wv) projective |= wave_flag[wv] != 0;
    return projective;
}
template <uint32_t WPB>
__device__ __forceinline__ bool block_projective(bool pj, uint32_t* wave_flag, uint32_t lane, uint32_t wave) {
    publish_projective(pj, wave_flag, lane, wave);
    __syncthreads();
    return read_projective<WPB>(wave_flag);
}

// Draw a unit from the workgroup's LDS ticket counter: one ds_add_rtn per wave, the value wave-uniform.
__device__ __forceinline__ uint32_t draw_ticket(uint32_t* ticket, uint32_t lane) {
    uint32_t t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(t);
}

// mat3 rows * v, reference order ((m0*x + m1*y) + m2*z); used by the projective normaliser.
template <bool EXACT>
__device__ __forceinline__ float dot3(f32x4 r, float x, float y, float z) {
    if constexpr (EXACT) return (r.x * x + r.y * y) + r.z * z;
    else return __builtin_fmaf(r.z, z, __builtin_fmaf(r.y, y, r.x * x));
}

// (a*x + b*y) + c*z on pairs; fused: fma(c, z, fma(b, y, a*x)).
template <bool EXACT>
__device__ __forceinline__ f32x2 dot3p(f32x2 a, f32x2 x, f32x2 b, f32x2 y, f32x2 c, f32x2 z) {
    if constexpr (EXACT) return (a * x + b * y) + c * z;
    else return __builtin_elementwise_fma(c, z, __builtin_elementwise_fma(b, y, a * x));
}
template <bool EXACT>
__device__ __forceinline__ f32x2 accp(f32x2 a, f32x2 r, f32x2 w) {
    if constexpr (EXACT) return a + r * w;
    else return __builtin_elementwise_fma(r, w, a);
}
template <bool EXACT>
__device__ __forceinline__ float acc(float a, float r, float w) {
    if constexpr (EXACT) return a + r * w;
    else return __builtin_fmaf(r, w, a);
}
__device__ __forceinline__ f32x2 splat(float v) { return f32x2{v, v}; }

struct Skinned {
    float px, py, pz, nx, ny, nz, tx, ty, tz;
};

// One vertex, four influences.  MASK bit0 position, bit1 normal, bit2 tangent.
// SEQ: the four influences one after another (three LDS rows live at a time instead of twelve: ~74 instead of ~112 VGPRs in
// the crowd kernel) -- the same operations in the same order per output component, so the same bits.
template <bool EXACT, int MASK, bool PROJ, bool SEQ = false>
__device__ __forceinline__ Skinned skin_vertex_impl(const f32x4* __restrict__ rows,
                                               const f32x4* __restrict__ row3,
                                               uint32_t id, f32x4 w, float px, float py, float pz,
                                               float nx, float ny, float nz, float tx, float ty,
                                               float tz) {
    f32x2 o_pxy = {0.f, 0.f}, o_x = {0.f, 0.f}, o_y = {0.f, 0.f}, o_z = {0.f, 0.f};  // o_r = (n_r, t_r)
    float o_pz = 0.f;
    const f32x2 vx = {nx, tx}, vy = {ny, ty}, vz = {nz, tz};
#pragma unroll(SEQ ? 1 : 4)
    for (int k = 0; k < 4; ++k) {
        const uint32_t b = (id >> (8 * k)) & 0xffu;
        const float wk = k == 0 ? w.x : k == 1 ? w.y : k == 2 ? w.z : w.w;
        const f32x4 A = rows[b * 3 + 0];
        const f32x4 B = rows[b * 3 + 1];
        const f32x4 C = rows[b * 3 + 2];
        if constexpr (MASK & 1) {
            f32x2 xy;
            float z;
            if constexpr (EXACT) {
                xy = dot3p<true>(A.xy, splat(px), A.zw, splat(py), B.xy, splat(pz)) + B.zw;
                z = ((C.x * px + C.y * py) + C.z * pz) + C.w;
            } else {
                xy = __builtin_elementwise_fma(
                    B.xy, splat(pz),
                    __builtin_elementwise_fma(A.zw, splat(py), __builtin_elementwise_fma(A.xy, splat(px), B.zw)));
                z = __builtin_fmaf(C.z, pz, __builtin_fmaf(C.y, py, __builtin_fmaf(C.x, px, C.w)));
            }
            if constexpr (PROJ) {
                const f32x4 r3 = row3[b];
                const float n = dot3<EXACT>(r3, px, py, pz) + r3.w;
                if (n != 0.0f) { xy.x = xy.x / n; xy.y = xy.y / n; z = z / n; }
            }
            o_pxy = accp<EXACT>(o_pxy, xy, splat(wk));
            o_pz = acc<EXACT>(o_pz, z, wk);
        }
        if constexpr ((MASK & 6) != 0) {
            // (n_r, t_r) for r = x, y, z; with only one of the two streams present the other lane
            // carries zeros and is never stored.
            const f32x2 rx = dot3p<EXACT>(splat(A.x), vx, splat(A.z), vy, splat(B.x), vz);
            const f32x2 ry = dot3p<EXACT>(splat(A.y), vx, splat(A.w), vy, splat(B.y), vz);
            const f32x2 rz = dot3p<EXACT>(splat(C.x), vx, splat(C.y), vy, splat(C.z), vz);
            o_x = accp<EXACT>(o_x, rx, splat(wk));
            o_y = accp<EXACT>(o_y, ry, splat(wk));
            o_z = accp<EXACT>(o_z, rz, splat(wk));
        }
    }
    Skinned o;
    o.px = o_pxy.x; o.py = o_pxy.y; o.pz = o_pz;
    o.nx = o_x.x; o.ny = o_y.x; o.nz = o_z.x;
    o.tx = o_x.y; o.ty = o_y.y; o.tz = o_z.y;
    return o;
}

// Fused mode for VALU-bound launches (crowds): blend the four matrices first, M = sum_k w_k M_k, then transform
// position / normal / tangent once.  For affine palettes this is the same linear map as sum_k (M_k v) w_k -- only
// the rounding differs (a few 1e-7 relative, inside the 1e-5 bar of lbs.exact=0) -- and costs ~40 packed VALU
// instead of ~138: 24 for the blend (three float4 per bone, two pk-FMAs each) and 15 for the three transforms.
template <int MASK>
__device__ __forceinline__ Skinned skin_vertex_blended(const f32x4* __restrict__ rows, uint32_t id, f32x4 w, float px,
                                                       float py, float pz, float nx, float ny, float nz, float tx,
                                                       float ty, float tz) {
    f32x2 a_lo, a_hi, b_lo, b_hi, c_lo, c_hi;
    {
        const uint32_t b0 = id & 0xffu;
        const f32x4 A = rows[b0 * 3 + 0], B = rows[b0 * 3 + 1], C = rows[b0 * 3 + 2];
        const f32x2 ww = splat(w[0]);
        a_lo = A.xy * ww; a_hi = A.zw * ww; b_lo = B.xy * ww; b_hi = B.zw * ww; c_lo = C.xy * ww; c_hi = C.zw * ww;
    }
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const uint32_t b = (id >> (8 * k)) & 0xffu;
        const f32x4 A = rows[b * 3 + 0], B = rows[b * 3 + 1], C = rows[b * 3 + 2];
        const f32x2 ww = splat(w[k]);
        a_lo = __builtin_elementwise_fma(A.xy, ww, a_lo); a_hi = __builtin_elementwise_fma(A.zw, ww, a_hi);
        b_lo = __builtin_elementwise_fma(B.xy, ww, b_lo); b_hi = __builtin_elementwise_fma(B.zw, ww, b_hi);
        c_lo = __builtin_elementwise_fma(C.xy, ww, c_lo); c_hi = __builtin_elementwise_fma(C.zw, ww, c_hi);
    }
    // blended rows: (m00,m10) (m01,m11) (m02,m12) (t0,t1) (m20,m21) (m22,t2)
    Skinned o;
    o.px = o.py = o.pz = o.nx = o.ny = o.nz = o.tx = o.ty = o.tz = 0.f;
    if constexpr (MASK & 1) {
        const f32x2 xy = __builtin_elementwise_fma(b_lo, splat(pz), __builtin_elementwise_fma(a_hi, splat(py),
                         __builtin_elementwise_fma(a_lo, splat(px), b_hi)));
        o.px = xy.x; o.py = xy.y;
        o.pz = __builtin_fmaf(c_hi.x, pz, __builtin_fmaf(c_lo.y, py, __builtin_fmaf(c_lo.x, px, c_hi.y)));
    }
    if constexpr ((MASK & 6) != 0) {
        const f32x2 vx = {nx, tx}, vy = {ny, ty}, vz = {nz, tz};
        const f32x2 rx = __builtin_elementwise_fma(splat(b_lo.x), vz, __builtin_elementwise_fma(splat(a_hi.x), vy, splat(a_lo.x) * vx));
        const f32x2 ry = __builtin_elementwise_fma(splat(b_lo.y), vz, __builtin_elementwise_fma(splat(a_hi.y), vy, splat(a_lo.y) * vx));
        const f32x2 rz = __builtin_elementwise_fma(splat(c_hi.x), vz, __builtin_elementwise_fma(splat(c_lo.y), vy, splat(c_lo.x) * vx));
        o.nx = rx.x; o.ny = ry.x; o.nz = rz.x;
        o.tx = rx.y; o.ty = ry.y; o.tz = rz.y;
    }
    return o;
}

// `projective` is workgroup-uniform: the affine path (the only kind of palette Fyrox produces)
// is one straight-line block of packed math; the homogeneous divide lives in its own copy.
template <bool EXACT, int MASK, bool BLEND_FIRST = false, bool SEQ = false>
__device__ __forceinline__ Skinned skin_vertex(const f32x4* __restrict__ rows,
                                               const f32x4* __restrict__ row3, bool projective,
                                               uint32_t id, f32x4 w, float px, float py, float pz,
                                               float nx, float ny, float nz, float tx, float ty,
                                               float tz) {
    if (projective) return skin_vertex_impl<EXACT, MASK, true, SEQ>(rows, row3, id, w, px, py, pz, nx, ny, nz, tx, ty, tz);
    if constexpr (!EXACT && BLEND_FIRST) return skin_vertex_blended<MASK>(rows, id, w, px, py, pz, nx, ny, nz, tx, ty, tz);
    return skin_vertex_impl<EXACT, MASK, false, SEQ>(rows, row3, id, w, px, py, pz, nx, ny, nz, tx, ty, tz);
}

// p and n are kept as whole 96-bit values (one register triple each): a loop that carries a vertex from one
// iteration to the next then carries the triple a dwordx3 load fills, instead of six scalars the register allocator
// is free to scatter (and has to gather again with moves that wait for the load).
template <int MASK>
struct VertexIn {
    f32x3 p, n;
    f32x4 t, w;
    uint32_t id;
};

template <bool NT, int MASK>
__device__ __forceinline__ VertexIn<MASK> load_vertex(const LbsArgs& a, uint32_t vs) {
    VertexIn<MASK> r;
    r.p = r.n = f32x3{0.f, 0.f, 0.f};
    r.t = f32x4{0.f, 0.f, 0.f, 0.f};
    float x, y, z;
    if constexpr (MASK & 1) { ld3<NT>(a.pos + (size_t)vs * 3, x, y, z); r.p = f32x3{x, y, z}; }
    if constexpr (MASK & 2) { ld3<NT>(a.nrm + (size_t)vs * 3, x, y, z); r.n = f32x3{x, y, z}; }
    if constexpr (MASK & 4) r.t = ldg<NT>(reinterpret_cast<const f32x4*>(a.tan) + vs);
    r.w = ldg<NT>(reinterpret_cast<const f32x4*>(a.wgt) + vs);
    r.id = ldg<NT>(a.idx + vs);
    return r;
}

template <int MASK>
__device__ __forceinline__ void pin_vertex(VertexIn<MASK>& r) {
    asm volatile("" : "+v"(r.p), "+v"(r.n));
    asm volatile("" : "+v"(r.t), "+v"(r.w), "+v"(r.id));
}

// ---------------------------------------------------------------------------------------
// Vertex streams as buffer resources (lbs_skin_dyn): buffer_load / buffer_store carry the cache policy in the
// instruction (aux bits below), the compiler knows them (exact vmcnt counts, hazards), and an access past the
// stream's last byte is dropped by the hardware (loads return 0) -- no per-lane bounds test.
//   aux: 1 = sc0, 2 = nt, 16 = sc1   (gfx940+ cache-policy bits of the raw-buffer builtins)
// ---------------------------------------------------------------------------------------
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
struct VtxBuffers {
    __amdgpu_buffer_rsrc_t pos, nrm, tan, wgt, idx, out_pos, out_nrm, out_tan;
};
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_stream(const void* p, uint32_t bytes) {
    // null stream -> zero records: every access is out of range
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, p ? bytes : 0u, 0x00020000);
}
__device__ __forceinline__ VtxBuffers make_vtx_buffers(const LbsArgs& a) {
    VtxBuffers b;
    b.pos = make_stream(a.pos, a.n_verts * 12u);
    b.nrm = make_stream(a.nrm, a.n_verts * 12u);
    b.tan = make_stream(a.tan, a.n_verts * 16u);
    b.wgt = make_stream(a.wgt, a.n_verts * 16u);
    b.idx = make_stream(a.idx, a.n_verts * 4u);
    b.out_pos = make_stream(a.out_pos, a.n_verts * 12u);
    b.out_nrm = make_stream(a.out_nrm, a.n_verts * 12u);
    b.out_tan = make_stream(a.out_tan, a.n_verts * 16u);
    return b;
}
template <int MASK, int AUX>
__device__ __forceinline__ VertexIn<MASK> load_vertex_buf(const VtxBuffers& b, uint32_t v) {
    VertexIn<MASK> r;
    r.p = r.n = f32x3{0.f, 0.f, 0.f};
    r.t = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (MASK & 1) r.p = __builtin_bit_cast(f32x3, __builtin_amdgcn_raw_buffer_load_b96(b.pos, v * 12u, 0, AUX));
    if constexpr (MASK & 2) r.n = __builtin_bit_cast(f32x3, __builtin_amdgcn_raw_buffer_load_b96(b.nrm, v * 12u, 0, AUX));
    if constexpr (MASK & 4) r.t = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(b.tan, v * 16u, 0, AUX));
    r.w = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(b.wgt, v * 16u, 0, AUX));
    r.id = __builtin_amdgcn_raw_buffer_load_b32(b.idx, v * 4u, 0, AUX);
    return r;
}
template <int MASK, int AUX>
__device__ __forceinline__ void store_vertex_buf(const VtxBuffers& b, uint32_t v, const Skinned& o, float tw) {
    if constexpr (MASK & 1)
        __builtin_amdgcn_raw_buffer_store_b96(__builtin_bit_cast(u32x3, f32x3{o.px, o.py, o.pz}), b.out_pos, v * 12u, 0, AUX);
    if constexpr (MASK & 2)
        __builtin_amdgcn_raw_buffer_store_b96(__builtin_bit_cast(u32x3, f32x3{o.nx, o.ny, o.nz}), b.out_nrm, v * 12u, 0, AUX);
    if constexpr (MASK & 4)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{o.tx, o.ty, o.tz, tw}), b.out_tan, v * 16u, 0, AUX);
}

// ---------------------------------------------------------------------------------------
// Boxes of skinned positions inside the skinning kernels (the *_bounds forms, fyx_lbs_skin_ex_bounds).
// The reference's fold (AxisAlignedBoundingBox::add_point, fyrox-math/src/aabb.rs:33-104) starts from (+MAX, -MAX) and moves a
// bound on a strict < / >: a NaN component never enters, infinities do.  Here the six bounds are all kept as MINIMA --
// (min x, min y, min z, -max x, -max y, -max z) -- so every update is one v_min_f32 (the max half takes its source negated) and
// every reduction step is the same operation.  minnum(bound, NaN) is the bound (the positions are arithmetic results: quiet
// NaNs), minnum(+MAX, +inf) is +MAX as +inf < +MAX is false: the same fold, except for the sign of a zero bound, which the
// reference's own answer leaves to the visiting order.
// ---------------------------------------------------------------------------------------
struct BoxAcc {
    float v[6];
    __device__ __forceinline__ void reset() {
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = __FLT_MAX__;
    }
    __device__ __forceinline__ void add(float x, float y, float z) {
        v[0] = __builtin_fminf(v[0], x); v[1] = __builtin_fminf(v[1], y); v[2] = __builtin_fminf(v[2], z);
        v[3] = __builtin_fminf(v[3], -x); v[4] = __builtin_fminf(v[4], -y); v[5] = __builtin_fminf(v[5], -z);
    }
};

// LDS of one workgroup's boxes: component k of wave j's 64 lanes is the run of 64 floats at chunk k * WPB + j, chunks
// kBoxChunk floats apart (64 + 4: the 16 folding lanes of a b128 read start 16 bytes apart, every bank once).
constexpr uint32_t kBoxChunk = 68;
template <int BLOCK>
constexpr size_t box_lds_bytes() { return (size_t)6 * (BLOCK / 64) * kBoxChunk * sizeof(float); }

template <int BLOCK>
__device__ __forceinline__ void box_put(const BoxAcc& b, float* lds, uint32_t wave, uint32_t lane) {
    constexpr uint32_t WPB = BLOCK / 64;
#pragma unroll
    for (int k = 0; k < 6; ++k) lds[((uint32_t)k * WPB + wave) * kBoxChunk + lane] = b.v[k];
}

// One wave folds what box_put left (after a barrier) into the workgroup's partial box out6 = {min xyz, max xyz}: lane k * WPB + j
// takes wave j's 64 values of component k, then the WPB lanes of a component meet by shuffles.
template <int BLOCK>
__device__ __forceinline__ void box_fold(const float* lds, float* out6, uint32_t lane) {
    constexpr uint32_t WPB = BLOCK / 64;
    const uint32_t k = lane / WPB;
    float m = __FLT_MAX__;
    if (k < 6) {
        const f32x4* p = reinterpret_cast<const f32x4*>(lds + lane * kBoxChunk);
        // four b128 reads in flight at a time: the fold runs inside the skinning kernels, whose register budgets have no 64 VGPRs to spare
#pragma unroll 1
        for (int i = 0; i < 16; i += 4) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 q = p[i + r];
                m = __builtin_fminf(m, __builtin_fminf(__builtin_fminf(q.x, q.y), __builtin_fminf(q.z, q.w)));
            }
        }
    }
#pragma unroll
    for (uint32_t o = 1; o < WPB; o <<= 1) m = __builtin_fminf(m, __shfl_xor(m, (int)o, 64));
    if (k < 6 && lane % WPB == 0) out6[k] = k < 3 ? m : -m;
}

// The end of one (workgroup, instance) segment of a kernel that has no barrier there: every thread calls it.  The LDS is rewritten
// only after the barrier that starts the workgroup's next segment (palette staging), which wave 0 reaches after its fold.
template <int BLOCK>
__device__ __forceinline__ void box_segment_end(const BoxAcc& b, float* lds, float* out6, uint32_t wave, uint32_t lane) {
    box_put<BLOCK>(b, lds, wave, lane);
    __syncthreads();
    if (wave == 0) box_fold<BLOCK>(lds, out6, lane);
}

}  // namespace fyx
