"""The device-buffer trace calls of all four aggregate methods (wf_trace_closest_device_t, wf_trace_any_device_t,
wf_trace_shadow_tr_device, wf_trace_one_random_device): declared, exported, refusing a null context without touching a device, and
bound by wfpt.Scene.  What they compute is checked on the GPU (tests/test_device_trace_gpu.py)."""
import ctypes as C
import os
import re

from conftest import ROOT

NEW = ["wf_trace_closest_device_t", "wf_trace_any_device_t", "wf_trace_shadow_tr_device", "wf_trace_one_random_device"]
N_POINTERS = {"wf_trace_closest_device_t": 2, "wf_trace_any_device_t": 2, "wf_trace_shadow_tr_device": 7, "wf_trace_one_random_device": 4}


def test_header_declares_and_library_exports_the_four_calls(wfpt):
    text = open(os.path.join(ROOT, "include", "wf_abi.h")).read()
    _, hip = wfpt.libs()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(\s*wf_ctx\s*\*ctx,\s*int n," % name, text), name
        assert hasattr(hip, name), name
        assert name in wfpt.ABI_SYMBOLS, name


def test_abi_version_is_unchanged(wfpt):
    _, hip = wfpt.libs()
    assert hip.wf_abi_version() == 12
    assert re.search(r"#define\s+WF_ABI_VERSION\s+12\b", open(os.path.join(ROOT, "include", "wf_abi.h")).read())


def test_a_null_context_is_refused_with_a_message(wfpt):
    """no device is needed to be told so: the check comes before anything touches the runtime"""
    _, hip = wfpt.libs()
    for name in NEW:
        f = getattr(hip, name)
        f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * N_POINTERS[name]
        f.restype = C.c_int
        for n in (0, 1, 64):
            assert f(None, n, *([None] * N_POINTERS[name])) != 0, (name, n)
            msg = hip.wf_last_error().decode()
            assert msg and name in msg, (name, msg)


def test_scene_binds_the_three_methods(wfpt):
    for m in ("trace_device", "trace_shadow_tr_device", "trace_one_random_device"):
        assert callable(getattr(wfpt.Scene, m, None)), m
    assert callable(wfpt.hit_records)
    assert wfpt.HIT_DTYPE.itemsize == 32 and wfpt.HIT_DTYPE.names[0] == "prim" and wfpt.HIT_DTYPE.names[-1] == "instance"
