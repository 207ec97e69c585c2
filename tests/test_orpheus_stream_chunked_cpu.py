"""Chunked audio out of the Orpheus continuous session, without a device: the C ABI declares and exports the three new entry points, libtts.so
calls them, hip.py binds them, every one answers a NULL context with an error that names it, and the session's chunk hook is overridden once,
in host/stream_session.h, the base the three session runners share; orpheus_runner supplies its part, session_chunks_ready."""
import ctypes as C
import os
import re

from tts_cpp_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tts_hip_orpheus_stream_launch", "tts_hip_orpheus_stream_wait", "tts_hip_orpheus_stream_drop"]
HOST = os.path.join(ROOT, "tts.cpp_amd", "host")


def _without_comments(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_libraries_export_the_new_entry_points():
    assert os.path.exists(hip.lib_path()), "libtts_hip.so not built (run __graft_entry__.build())"
    L = C.CDLL(hip.lib_path())
    for name in NAMES:
        assert hasattr(L, name), f"{name} not exported"
        assert name in hip.EXPORTS
    host = os.path.join(HOST, "libtts.so")
    assert os.path.exists(host), "libtts.so not built"
    blob = open(host, "rb").read()
    for name in NAMES:                                                  # the runner's session calls all three
        assert name.encode() in blob, name


def test_header_declares_them_and_states_the_contract():
    hdr = _without_comments(os.path.join(ROOT, "include", "tts_hip.h"))
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*tts_hip_ctx\s*\*" % name, hdr), f"{name} not declared"
    full = open(os.path.join(ROOT, "include", "tts_hip.h")).read()
    at = full.index("int tts_hip_orpheus_stream_begin")
    comment = full[full.rindex("/*", 0, at):at]
    for word in ("launch", "wait", "drop", "without gap or overlap", "whatever the launch sizes", "run and collect return", "no other slot", "in flight",
                 "256 keys", "upper bound", "generate_batch"):            # the last three: the sentences test_orpheus_stream_cpu.py reads stay
        assert word in comment, word


def test_engine_has_the_methods():
    for m in ("stream_launch", "stream_wait", "stream_drop"):
        assert callable(getattr(hip.OrpheusEngine, m, None)), m


def test_new_entry_points_refuse_a_null_context():
    L = hip.load_lib()
    n = C.c_uint32()
    buf = (C.c_uint32 * 4)()
    assert L.tts_hip_orpheus_stream_launch(None, 1) != 0
    assert b"Orpheus context" in L.tts_hip_last_error() and b"tts_hip_orpheus_stream_launch" in L.tts_hip_last_error()
    assert L.tts_hip_orpheus_stream_wait(None, None, None, None, C.byref(n), buf, buf) != 0
    assert b"tts_hip_orpheus_stream_wait" in L.tts_hip_last_error()
    assert L.tts_hip_orpheus_stream_drop(None, 1, buf) != 0
    assert b"tts_hip_orpheus_stream_drop" in L.tts_hip_last_error()


def test_orpheus_session_header_declares_the_override():
    """an Orpheus runner cannot be loaded without a device, so the override is checked where it is declared"""
    session_h = open(os.path.join(HOST, "stream_session.h")).read()
    assert len(re.findall(r"\bbool\s+stream_chunks\([^;]*\)\s+override\s*;", session_h)) == 1
    assert re.search(r"struct\s+stream_session\s*:\s*tts_generation_runner\b", session_h)
    assert re.search(r"virtual\s+bool\s+session_chunks_ready\([^;]*\)\s*=\s*0\s*;", session_h)
    runner_h = open(os.path.join(HOST, "orpheus_runner.h")).read()
    assert '#include "stream_session.h"' in runner_h
    assert re.search(r"struct\s+orpheus_runner\s+final\s*:\s*stream_session\b", runner_h)
    assert re.search(r"\bbool\s+session_chunks_ready\([^;]*\)\s+override\s*;", runner_h)
    assert not re.search(r"\bstream_chunks\s*\(", open(os.path.join(HOST, "orpheus_runner.cpp")).read())   # no hook of its own beside the base's
    common = open(os.path.join(HOST, "common.h")).read()
    at = common.index("virtual bool     stream_chunks(")
    note = common[common.rindex("// chunked audio out of a session", 0, at):at]
    assert "orpheus_runner" in note and "dia_runner" in note and "parler_runner" in note
    assert re.search(r"does not chunk \(parler_runner\)", note), "Orpheus' session chunks now"
