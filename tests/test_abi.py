"""The C-ABI library loads, exports every symbol include/fyrox_hip.h declares, and fails LOUDLY
(no CPU fallback) when there is no GPU.  No compute calls here."""
import ctypes
import os
import re

import pytest

import fyrox_amd
from fyrox_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    names = set()
    for fn in os.listdir(os.path.join(ROOT, "include")):
        if fn.endswith(".h"):
            src = open(os.path.join(ROOT, "include", fn)).read()
            src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
            names |= set(re.findall(r"\b(fyx_[a-z0-9_]+)\s*\(", src))
    return names


def test_library_is_built_in_tree():
    assert os.path.exists(fyrox_amd.LIB_PATH), "run __graft_entry__.build()"
    assert os.path.dirname(fyrox_amd.LIB_PATH) == os.path.join(ROOT, "fyrox_amd")


def test_every_declared_symbol_is_exported_and_bound():
    declared = _declared_symbols()
    assert len(declared) >= 20
    raw = ctypes.CDLL(fyrox_amd.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(raw, name), f"{name} declared in include/*.h but not exported"
    assert declared == set(_native.exported_symbols()), declared ^ set(_native.exported_symbols())
    _native.lib()  # binds argtypes for every symbol; AttributeError if one is missing


def test_version_string():
    assert b"gfx950" in _native.lib().fyx_version()


def test_code_object_targets_gfx950_only():
    data = open(fyrox_amd.LIB_PATH, "rb").read()
    assert b"gfx950" in data
    for other in (b"gfx90a", b"gfx942", b"sm_80", b"nvptx"):
        assert other not in data


def test_product_never_references_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "fyrox_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")) or f == "Makefile":
                src = open(os.path.join(dirpath, f)).read()
                assert "fyrox_oracle" not in src, f
                assert not re.search(r"^\s*(import oracle|from oracle)", src, flags=re.M), f
    ldd = os.popen(f"objdump -p {fyrox_amd.LIB_PATH}").read()
    assert "oracle" not in ldd


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_no_gpu_fails_loudly_instead_of_falling_back():
    with pytest.raises(fyrox_amd.FyxError) as e:
        fyrox_amd.Context(0)
    assert e.value.code == _native.FYX_ERR_NO_DEVICE
    assert "no CPU fallback" in str(e.value)


def test_null_context_is_rejected_not_crashing():
    l = _native.lib()
    assert l.fyx_sync(None) == _native.FYX_ERR_INVALID_ARG
    assert l.fyx_mesh_free(None, 1) == _native.FYX_ERR_INVALID_ARG
    assert l.fyx_lbs_skin(None, 1, None, 1, 1, None, None, None, None) == _native.FYX_ERR_INVALID_ARG
    assert l.fyx_last_error(None) == b"null context"
    l.fyx_shutdown(None)


def test_rust_ffi_matches_header():
    """bindings/rust/fyrox_hip_sys.rs (the `extern "C"` block a Fyrox maintainer adds) is generated from
    include/fyrox_hip.h; it must be current and declare every exported symbol."""
    import subprocess
    import sys
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py"), "--check"]) == 0, \
        "bindings/rust/fyrox_hip_sys.rs is stale: run python tools/gen_rust_ffi.py"
    rs = open(os.path.join(ROOT, "bindings", "rust", "fyrox_hip_sys.rs")).read()
    assert set(re.findall(r"pub fn (fyx_[a-z0-9_]+)", rs)) == _declared_symbols()
    for st in ("FyxSkinDesc", "FyxTransform", "FyxTrackDesc", "FyxRootMotion", "FyxLayerEvent"):
        assert f"pub struct {st} " in rs


@pytest.mark.skipif(not os.path.isdir(os.environ.get("FYROX_SRC", "")),
                    reason="needs a checkout of the Fyrox sources named by FYROX_SRC, not part of this repository")
def test_rust_shim_uses_only_names_the_reference_has():
    """bindings/rust/fyrox_hip.rs and fyrox_hip_flatten.rs cannot be compiled here (no rustc); tools/lint_rust_shim.py
    checks every `crate::` path, every method / field / enum variant used on a reference type and every extern name against
    the Fyrox sources and the generated FFI block (the first version of the shim called VertexBuffer::find_attribute,
    which does not exist)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lint_rust_shim.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout


def test_options_are_validated_and_readable_without_a_gpu():
    """fyx_set_option / fyx_get_option on a control-only context: known keys round-trip, out-of-range values and unknown
    keys are error codes (the header lists the keys), and nothing needs a device."""
    import fyrox_amd
    c = fyrox_amd.Context(control_only=True)
    try:
        for key, good, bad in (("lbs.exact", 0, None), ("lbs.streams", 1, 9), ("lbs.crowd", -1, 2), ("lbs.crowd_ipb", 8, 5000),
                               ("lbs.blocks_per_cu", 2, 65), ("lbs.dyn", 0, None), ("anim.threads", 3, 0), ("anim.split", 64, 0),
                               ("anim.sample_form", 2, 3), ("anim.overlap", 1, 2), ("debug.overlap", 2, 3), ("anim.frame_skin", 1, 2), ("debug.frame_skin", 3, 4), ("anim.inline_ctrl", 0, 2), ("comm.form", 2, 3),
                                   ("anim.ctrl_upload", 0, 3), ("anim.update_lean", 0, 2), ("anim.update_pack", 2, 3), ("anim.one_launch", 0, 2), ("debug.timeline", 0, None),
                               ("lbs.timing", 1, None)):
            if key == "lbs.streams":
                continue      # binds the device when it changes: a data-path option
            c.set_option(key, good)
            assert c.get_option(key) == good, key
            if bad is not None:
                with pytest.raises(fyrox_amd.FyxError):
                    c.set_option(key, bad)
                assert c.get_option(key) == good, key
        with pytest.raises(fyrox_amd.FyxError):
            c.set_option("no.such.option", 1)
        with pytest.raises(fyrox_amd.FyxError):
            c.get_option("no.such.option")
    finally:
        c.close()


def test_one_process_exchange_refuses_contexts_without_a_gpu():
    """fyx_comm_init_all / fyx_allgather_skinned_all: argument errors are error codes on ctxs[0], nothing needs a device."""
    import ctypes
    import fyrox_amd
    from fyrox_amd import _native
    a, b = fyrox_amd.Context(control_only=True), fyrox_amd.Context(control_only=True)
    try:
        with pytest.raises(fyrox_amd.FyxError) as e:
            fyrox_amd.Context.comm_init_all([a, b])
        assert e.value.code == _native.FYX_ERR_NO_DEVICE
        with pytest.raises(fyrox_amd.FyxError):
            fyrox_amd.Context.allgather_skinned_all([a], 100, [0], None, None)       # no communicator
        lib = _native.lib()
        assert lib.fyx_comm_init_all(None, 1) == _native.FYX_ERR_INVALID_ARG
        arr = (ctypes.c_void_p * 2)(a._h, None)
        assert lib.fyx_comm_init_all(arr, 2) == _native.FYX_ERR_INVALID_ARG
        assert lib.fyx_comm_init_all(arr, 0) == _native.FYX_ERR_INVALID_ARG
        assert lib.fyx_allgather_skinned_all(arr, 2, 10, None, None, None) == _native.FYX_ERR_INVALID_ARG
    finally:
        a.close()
        b.close()
