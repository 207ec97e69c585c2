"""The Orpheus continuous session without a device: the C ABI declares and exports it, hip.py binds it, and the host headers no longer
describe continuous batching as Parler's alone."""
import ctypes as C
import os
import re

from tts_cpp_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tts_hip_orpheus_stream_begin", "tts_hip_orpheus_stream_admit", "tts_hip_orpheus_stream_run", "tts_hip_orpheus_stream_collect",
         "tts_hip_orpheus_stream_end", "tts_hip_orpheus_sample_logits_rows"]


def _without_comments(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_header_declares_and_library_exports_the_session():
    hdr = _without_comments(os.path.join(ROOT, "include", "tts_hip.h"))
    assert os.path.exists(hip.lib_path()), "libtts_hip.so not built (run __graft_entry__.build())"
    L = C.CDLL(hip.lib_path())
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*tts_hip_ctx\s*\*" % name, hdr), f"{name} not declared"
        assert name in hip.EXPORTS
        assert hasattr(L, name), f"{name} not exported"


def test_session_comment_carries_the_key_split_caveat():
    hdr = open(os.path.join(ROOT, "include", "tts_hip.h")).read()
    at = hdr.index("int tts_hip_orpheus_stream_begin")
    comment = hdr[hdr.rindex("/*", 0, at):at]
    assert "256 keys" in comment and "upper bound" in comment and "generate_batch" in comment


def test_engine_has_the_session_methods():
    for m in ("stream_begin", "stream_admit", "stream_run", "stream_collect", "stream_end", "sample_logits_rows"):
        assert callable(getattr(hip.OrpheusEngine, m, None)), m


def test_session_errors_without_a_context():
    """the entry points answer a NULL context with an error, not a crash"""
    L = hip.load_lib()
    n = C.c_uint32()
    buf = (C.c_uint32 * 4)()
    assert L.tts_hip_orpheus_stream_begin(None, 2, 8, 0, None) != 0
    assert b"Orpheus context" in L.tts_hip_last_error()
    assert L.tts_hip_orpheus_stream_run(None, 1, C.byref(n), buf, buf) != 0
    assert L.tts_hip_orpheus_stream_collect(None, 0, 0, buf) != 0
    assert L.tts_hip_orpheus_stream_end(None) != 0


def test_host_headers_describe_the_orpheus_session():
    tts_c = open(os.path.join(ROOT, "include", "tts_c.h")).read()
    at = tts_c.index("tts_c_generate_stream(")
    comment = tts_c[tts_c.rindex("/*", 0, at):at]
    assert "Orpheus" in comment and "finish" in comment and "TTS_SNAC_NO_NOISE" in comment
    common = open(os.path.join(ROOT, "tts.cpp_amd", "host", "common.h")).read()
    at = common.index("struct stream_result")
    block = common[common.rindex("continuous batching", 0, at):at]
    assert "orpheus_runner" in block and "utterances finish" in block
    runner_h = open(os.path.join(ROOT, "tts.cpp_amd", "host", "orpheus_runner.h")).read()
    assert "stream_capacity() const override" in runner_h
