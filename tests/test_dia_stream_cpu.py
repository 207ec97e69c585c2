"""The Dia continuous session without a device: the C ABI declares and exports it, hip.py binds it, the runner overrides the session interface
and the host headers list Dia among the runners that have one."""
import ctypes as C
import os
import re

from tts_cpp_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tts_hip_dia_stream_begin", "tts_hip_dia_stream_admit", "tts_hip_dia_stream_run", "tts_hip_dia_stream_collect", "tts_hip_dia_stream_end"]


def _without_comments(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_library_exports_the_session():
    assert os.path.exists(hip.lib_path()), "libtts_hip.so not built (run __graft_entry__.build())"
    L = C.CDLL(hip.lib_path())
    for name in NAMES:
        assert hasattr(L, name), f"{name} not exported"
        assert name in hip.EXPORTS


def test_header_declares_the_session_and_states_its_contract():
    hdr = _without_comments(os.path.join(ROOT, "include", "tts_hip.h"))
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*tts_hip_ctx\s*\*" % name, hdr), f"{name} not declared"
    full = open(os.path.join(ROOT, "include", "tts_hip.h")).read()
    at = full.index("int tts_hip_dia_stream_begin")
    comment = full[full.rindex("/*", 0, at):at]
    for word in ("Fixed shape", "Parking", "Equality", "n_utt = n_slots", "refused", "budget"):
        assert word in comment, word


def test_engine_has_the_session_methods():
    for m in ("stream_begin", "stream_admit", "stream_run", "stream_collect", "stream_end"):
        assert callable(getattr(hip.DiaEngine, m, None)), m


def test_session_errors_without_a_context():
    """the entry points answer a NULL context with an error, not a crash"""
    L = hip.load_lib()
    n = C.c_uint32()
    buf = (C.c_uint32 * 4)()
    assert L.tts_hip_dia_stream_begin(None, 2, 8, None, None) != 0
    assert b"Dia context" in L.tts_hip_last_error()
    assert L.tts_hip_dia_stream_admit(None, 1, buf, buf, buf, None, None) != 0
    assert L.tts_hip_dia_stream_run(None, 1, C.byref(n), buf, buf) != 0
    assert L.tts_hip_dia_stream_collect(None, 0, 0, buf) != 0
    assert L.tts_hip_dia_stream_end(None) != 0


def test_runner_overrides_the_session_interface():
    """a Dia runner cannot be loaded without a device (its contexts are created at load), so the override is checked where it is declared"""
    runner_h = open(os.path.join(ROOT, "tts.cpp_amd", "host", "dia_runner.h")).read()
    assert re.search(r"uint32_t\s+stream_capacity\(\)\s+const\s+override\s*\{\s*return\s+max_seqs\s*>\s*1\s*\?\s*max_seqs\s*:\s*0;", runner_h)
    for m in ("stream_begin", "stream_free", "stream_live", "stream_submit", "stream_step", "stream_end"):
        assert re.search(r"\b%s\([^)]*\)(\s+const)?\s+override" % m, runner_h), m
    lib = os.path.join(ROOT, "tts.cpp_amd", "host", "libtts.so")
    assert os.path.exists(lib), "libtts.so not built"
    assert b"tts_hip_dia_stream_admit" in open(lib, "rb").read()        # the runner calls into the session


def test_host_headers_list_dia_among_the_sessions():
    tts_c = open(os.path.join(ROOT, "include", "tts_c.h")).read()
    at = tts_c.index("tts_c_generate_stream(")
    comment = tts_c[tts_c.rindex("/*", 0, at):at]
    assert "Dia: max_seqs utterances" in comment and "Dia and Kokoro have no session" not in comment
    common = open(os.path.join(ROOT, "tts.cpp_amd", "host", "common.h")).read()
    at = common.index("struct stream_result")
    block = common[common.rindex("continuous batching", 0, at):at]
    assert "dia_runner: every 16 steps" in block
    pool_h = open(os.path.join(ROOT, "tts.cpp_amd", "host", "device_pool.h")).read()
    assert "dia_runner every 16 steps" in pool_h
