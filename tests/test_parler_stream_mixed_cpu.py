"""The Parler mixed session (per-request sampler and seed in one lock-step loop), the parts that need no device: the two new C symbols are
exported, declared and listed, the header states the contract, each refuses a NULL context by name, hip.py binds them and parler_runner
overrides the two per-request virtuals."""
import ctypes
import os
import re

from tts_cpp_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_NEW = ["tts_hip_parler_stream_begin_mixed", "tts_hip_parler_stream_admit_mixed"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _without_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_libraries_export_list_and_reference_the_new_symbols():
    assert os.path.exists(hip.lib_path()), "libtts_hip.so not built"
    L = ctypes.CDLL(hip.lib_path())
    host = os.path.join(ROOT, "tts.cpp_amd", "host", "libtts.so")
    assert os.path.exists(host), "libtts.so not built"
    blob = open(host, "rb").read()
    for name in HIP_NEW:
        assert hasattr(L, name), f"{name} not exported"
        assert name in hip.EXPORTS, name
        assert name.encode() in blob, f"libtts.so does not reference {name}"   # the runner's session calls both


def test_header_declares_them_and_states_the_contract():
    full = _read("include", "tts_hip.h")
    hdr = _without_comments(full)
    assert re.search(r"\bint\s+tts_hip_parler_stream_begin_mixed\s*\(\s*tts_hip_ctx\s*\*ctx,\s*uint32_t n_slots,\s*uint32_t max_steps,\s*uint32_t bos,\s*uint32_t eos\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+tts_hip_parler_stream_admit_mixed\s*\(\s*tts_hip_ctx\s*\*ctx,\s*uint32_t n,\s*const uint32_t \*slots,\s*const uint32_t \*ids,\s*"
                     r"const uint32_t \*lens,\s*const tts_hip_sampling \*const \*sampling,\s*const float \*uniforms\s*\)\s*;", hdr)
    at = full.index("int tts_hip_parler_stream_begin(")
    comment = full[full.rindex("/*", 0, at):at]
    for word in ("sampler::max", "[n][max_steps][heads]", "[max_steps + 1][n_slots + 1][heads]", "session unchanged",
                 "an utterance's tokens and step count are those of tts_hip_parler_generate_greedy / tts_hip_parler_generate_sampled",
                 "whoever else is live, greedy or sampled, and whenever it entered", "recaptures", "tile shape"):
        assert word in comment, word


def test_each_refuses_a_null_context_by_name():
    L = hip.load_lib()
    calls = {
        "tts_hip_parler_stream_begin_mixed": lambda: L.tts_hip_parler_stream_begin_mixed(None, 2, 32, 1025, 1024),
        "tts_hip_parler_stream_admit_mixed": lambda: L.tts_hip_parler_stream_admit_mixed(None, 0, None, None, None, None, None),
    }
    assert sorted(calls) == sorted(HIP_NEW)
    for name, call in calls.items():
        assert call() != 0, name
        assert name in L.tts_hip_last_error().decode("utf-8", "replace"), name


def test_engine_binds_the_two_calls():
    for name in ("stream_begin_mixed", "stream_admit_mixed"):
        assert callable(getattr(hip.HipEngine, name, None)), name


def test_parler_runner_overrides_the_per_request_virtuals():
    """... and its session hands out whole utterances unless chunks are opted into: the behaviour is held on the device by
    tests/test_gpu_dia_stream_chunked.py::test_sessions_that_do_not_chunk_hand_out_whole_utterances (Parler without TTS_PARLER_STREAM_CHUNKS);
    here common.h's note and the runner are checked to carry the switch"""
    text = _read("tts.cpp_amd", "host", "parler_runner.h")
    assert re.search(r"bool\s+stream_accepts\(const generation_configuration &\s*\w*\)\s*const\s+override;", text)
    assert re.search(r"void\s+stream_submit\(size_t \w+, const std::string &\s*\w+, const generation_configuration &\s*\w*\)\s*override;", text)
    common = _read("tts.cpp_amd", "host", "common.h")
    at = common.index("virtual bool     stream_chunks(")
    note = common[common.rindex("// chunked audio out of a session", 0, at):at]
    assert "TTS_PARLER_STREAM_CHUNKS" in note and "opt-in" in note and "does not chunk (parler_runner)" in note
    source = _read("tts.cpp_amd", "host", "parler_runner.cpp")
    ready = source[source.index("bool parler_runner::session_chunks_ready("):]
    assert re.search(r'getenv\("TTS_PARLER_STREAM_CHUNKS"\);\s*if \(!on \|\| !\*on \|\| !strcmp\(on, "0"\)\) return false;', ready[:ready.index("\n}\n")])
