"""Chunked audio out of the Dia continuous session, without a device: the C ABIs declare and export the new entry points, hip.py and runner.py
bind them, every one answers a NULL context with an error, and the Dia runner overrides the session's chunk hook."""
import ctypes as C
import os
import re

from tts_cpp_amd import hip, runner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tts_hip_dia_stream_launch", "tts_hip_dia_stream_wait", "tts_hip_dia_stream_drop"]


def _without_comments(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_libraries_export_the_new_entry_points():
    assert os.path.exists(hip.lib_path()), "libtts_hip.so not built (run __graft_entry__.build())"
    L = C.CDLL(hip.lib_path())
    for name in NAMES:
        assert hasattr(L, name), f"{name} not exported"
        assert name in hip.EXPORTS
    host = os.path.join(ROOT, "tts.cpp_amd", "host", "libtts.so")
    assert os.path.exists(host), "libtts.so not built"
    assert hasattr(C.CDLL(host), "tts_c_generate_stream_chunked")
    assert "tts_c_generate_stream_chunked" in runner.EXPORTS
    for name in NAMES:                                                  # the runner's session calls all three
        assert name.encode() in open(host, "rb").read(), name


def test_headers_declare_them_and_state_the_contract():
    hdr = _without_comments(os.path.join(ROOT, "include", "tts_hip.h"))
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*tts_hip_ctx\s*\*" % name, hdr), f"{name} not declared"
    full = open(os.path.join(ROOT, "include", "tts_hip.h")).read()
    at = full.index("int tts_hip_dia_stream_begin")
    comment = full[full.rindex("/*", 0, at):at]
    for word in ("launch", "wait", "drop", "without gap or overlap", "whatever the launch sizes", "changes no other slot", "in flight"):
        assert word in comment, word
    tts_c = _without_comments(os.path.join(ROOT, "include", "tts_c.h"))
    assert re.search(r"\bint\s+tts_c_generate_stream_chunked\s*\(\s*tts_c_runner\s*\*[^;]*uint32_t\s+chunk_frames\s*,\s*tts_c_chunk_fn\s+fn\s*,\s*void\s*\*\s*user\s*\)\s*;", tts_c)
    common = open(os.path.join(ROOT, "tts.cpp_amd", "host", "common.h")).read()
    assert re.search(r"virtual\s+bool\s+stream_chunks\(uint32_t chunk_frames,\s*std::function<bool\(size_t ticket, const float \*, size_t\)> on_chunk\);", common)
    assert re.search(r"\n\s+void\s+generate_stream_chunked\(", common)   # not virtual


def test_engine_and_runner_have_the_methods():
    for m in ("stream_launch", "stream_wait", "stream_drop"):
        assert callable(getattr(hip.DiaEngine, m, None)), m
    assert callable(getattr(runner.Runner, "generate_stream_chunked", None))


def test_new_entry_points_refuse_a_null_context():
    L = hip.load_lib()
    n = C.c_uint32()
    buf = (C.c_uint32 * 4)()
    assert L.tts_hip_dia_stream_launch(None, 1) != 0
    assert b"Dia context" in L.tts_hip_last_error()
    assert L.tts_hip_dia_stream_wait(None, None, None, None, C.byref(n), buf, buf) != 0
    assert b"tts_hip_dia_stream_wait" in L.tts_hip_last_error()
    assert L.tts_hip_dia_stream_drop(None, 1, buf) != 0
    assert b"tts_hip_dia_stream_drop" in L.tts_hip_last_error()
    R = runner.load_lib()
    fn = runner.CHUNK_FN(lambda user, utt, pcm, k: 1)
    arr = (C.c_char_p * 1)(b"[S1] hi.")
    assert R.tts_c_generate_stream_chunked(None, arr, 1, None, 8, fn, None) not in (0, 1)
    assert b"tts_c_generate_stream_chunked" in R.tts_c_last_error()


def test_dia_runner_overrides_the_chunk_hook():
    """a runner cannot be loaded without a device, so the override is checked where it is declared: once, in the base the three session runners
    share (host/stream_session.h), with each runner's part behind the pure session_chunks_ready.  Parler's part is an opt-in: that its session
    hands out whole utterances without TTS_PARLER_STREAM_CHUNKS is held on the device by
    tests/test_gpu_dia_stream_chunked.py::test_sessions_that_do_not_chunk_hand_out_whole_utterances; here the switch is checked to be in place."""
    host = os.path.join(ROOT, "tts.cpp_amd", "host")
    session_h = open(os.path.join(host, "stream_session.h")).read()
    assert len(re.findall(r"\bbool\s+stream_chunks\([^;]*\)\s+override\s*;", session_h)) == 1
    assert re.search(r"struct\s+stream_session\s*:\s*tts_generation_runner\b", session_h)
    assert re.search(r"virtual\s+bool\s+session_chunks_ready\([^;]*\)\s*=\s*0\s*;", session_h)
    for name in ("dia", "parler", "orpheus"):
        runner_h = open(os.path.join(host, name + "_runner.h")).read()
        assert '#include "stream_session.h"' in runner_h, name
        assert re.search(r"struct\s+%s_runner\s+final\s*:\s*stream_session\b" % name, runner_h), name
        assert re.search(r"\bbool\s+session_chunks_ready\([^;]*\)\s+override\s*;", runner_h), name
        assert not re.search(r"\bstream_chunks\s*\(", open(os.path.join(host, name + "_runner.cpp")).read()), name   # no hook of its own
    parler_cpp = open(os.path.join(host, "parler_runner.cpp")).read()
    ready = parler_cpp[parler_cpp.index("bool parler_runner::session_chunks_ready("):]
    ready = ready[:ready.index("\n}\n")]
    assert 'getenv("TTS_PARLER_STREAM_CHUNKS")' in ready and "return false" in ready
    common = open(os.path.join(host, "common.h")).read()
    at = common.index("virtual bool     stream_chunks(")
    note = common[common.rindex("// chunked audio out of a session", 0, at):at]
    assert "TTS_PARLER_STREAM_CHUNKS" in note and "opt-in" in note and "no halo" in note
