"""The Dia mixed session (per-request sampler, seed and length in one device loop), the parts that need no device: the three new C symbols
are exported, declared and listed, each refuses a NULL context by name, and dia_runner overrides the two per-request virtuals."""
import ctypes
import os
import re

from tts_cpp_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_NEW = ["tts_hip_dia_stream_begin_mixed", "tts_hip_dia_stream_admit_mixed", "tts_hip_sample_logits_rows_mixed"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_new_symbols_are_declared_listed_and_exported():
    text = _read("include", "tts_hip.h")
    L = ctypes.CDLL(os.path.join(ROOT, "tts.cpp_amd", "libtts_hip.so"))
    for name in HIP_NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(tts_hip_ctx \*ctx,", text), name
        assert name in hip.EXPORTS, name
        assert hasattr(L, name), name


def test_each_refuses_a_null_context_by_name():
    L = hip.load_lib()
    codes = hip.DiaCodes(1026, 1024, 1025, 15)
    calls = {
        "tts_hip_dia_stream_begin_mixed": lambda: L.tts_hip_dia_stream_begin_mixed(None, 2, 32, ctypes.byref(codes)),
        "tts_hip_dia_stream_admit_mixed": lambda: L.tts_hip_dia_stream_admit_mixed(None, 0, None, None, None, None, None, None),
        "tts_hip_sample_logits_rows_mixed": lambda: L.tts_hip_sample_logits_rows_mixed(None, 1, None, None, None, None, None, None),
    }
    assert sorted(calls) == sorted(HIP_NEW)
    for name, call in calls.items():
        assert call() != 0, name
        assert name in L.tts_hip_last_error().decode("utf-8", "replace"), name


def test_dia_runner_overrides_the_per_request_virtuals():
    text = _read("tts.cpp_amd", "host", "dia_runner.h")
    assert re.search(r"bool\s+stream_accepts\(const generation_configuration &\s*\w*\)\s*const\s+override;", text)
    assert re.search(r"void\s+stream_submit\(size_t \w+, const std::string &\s*\w+, const generation_configuration &\s*\w*\)\s*override;", text)
