"""Per-request voice descriptions, the parts that need no device: the new tts_hip_* / tts_c_* symbols are exported, declared and listed, each
refuses a NULL context by name, the header states the contract, common.h declares add_voice and parler_runner overrides it, and a runner
without voice descriptions (the weightless dummy) refuses add_voice and still keeps a differing voice out of its session."""
import ctypes
import os
import re

import pytest

from tts_cpp_amd import hip, runner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_NEW = ["tts_hip_parler_voice_bank", "tts_hip_parler_voice_set", "tts_hip_parler_seq_voices"]
C_NEW = ["tts_c_add_voice", "tts_c_list_voices", "tts_c_pool_add_voice"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _without_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_libraries_export_list_and_reference_the_new_symbols():
    assert os.path.exists(hip.lib_path()), "libtts_hip.so not built"
    L = ctypes.CDLL(hip.lib_path())
    assert os.path.exists(runner.lib_path()), "libtts.so not built"
    H = ctypes.CDLL(runner.lib_path())
    blob = open(runner.lib_path(), "rb").read()
    for name in HIP_NEW:
        assert hasattr(L, name), f"{name} not exported"
        assert name in hip.EXPORTS, name
        assert name.encode() in blob, f"libtts.so does not reference {name}"   # parler_runner calls all three
    for name in C_NEW:
        assert hasattr(H, name), f"{name} not exported"
        assert name in runner.EXPORTS, name


def test_headers_declare_them_and_state_the_contract():
    full = _read("include", "tts_hip.h")
    hdr = _without_comments(full)
    assert re.search(r"\bint\s+tts_hip_parler_voice_bank\s*\(\s*tts_hip_ctx\s*\*ctx,\s*uint32_t n_voices\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+tts_hip_parler_voice_set\s*\(\s*tts_hip_ctx\s*\*ctx,\s*uint32_t voice,\s*const float \*enc,\s*uint32_t n_tokens\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+tts_hip_parler_seq_voices\s*\(\s*tts_hip_ctx\s*\*ctx,\s*uint32_t n,\s*const uint32_t \*seqs,\s*const uint32_t \*voices\s*\)\s*;", hdr)
    at = full.index("int tts_hip_parler_voice_bank(")
    comment = full[full.rindex("/*", 0, at):at]
    for word in ("bit for bit", "32 positions", "never recaptures", "cross_fold", "voice 0", "before anything is launched", "voice:<v>:<layer>:<0|1>"):
        assert word in comment, word
    chdr = _without_comments(_read("include", "tts_c.h"))
    assert re.search(r"\bint\s+tts_c_add_voice\s*\(\s*tts_c_runner\s*\*r,\s*const char \*name,\s*const char \*text_encoder_path,\s*const char \*description\s*\)\s*;", chdr)
    assert re.search(r"\bint\s+tts_c_pool_add_voice\s*\(\s*tts_c_pool\s*\*pool,\s*const char \*name,\s*const char \*description\s*\)\s*;", chdr)
    assert re.search(r"\bint\s+tts_c_list_voices\s*\(", chdr)


def test_each_refuses_a_null_context_by_name():
    L = hip.load_lib()
    calls = {
        "tts_hip_parler_voice_bank": lambda: L.tts_hip_parler_voice_bank(None, 4),
        "tts_hip_parler_voice_set": lambda: L.tts_hip_parler_voice_set(None, 1, None, 8),
        "tts_hip_parler_seq_voices": lambda: L.tts_hip_parler_seq_voices(None, 0, None, None),
    }
    assert sorted(calls) == sorted(HIP_NEW)
    for name, call in calls.items():
        assert call() != 0, name
        assert name in L.tts_hip_last_error().decode("utf-8", "replace"), name
    H = runner.load_lib()
    assert H.tts_c_add_voice(None, b"a", b"x.gguf", b"calm") != 0 and b"tts_c_add_voice" in H.tts_c_last_error()
    assert H.tts_c_pool_add_voice(None, b"a", b"calm") < 0 and b"tts_c_pool_add_voice" in H.tts_c_last_error()
    assert H.tts_c_list_voices(None, None, 0) < 0 and b"tts_c_list_voices" in H.tts_c_last_error()


def test_engine_and_runner_bind_the_calls():
    for name in ("voice_bank", "voice_set", "seq_voices"):
        assert callable(getattr(hip.HipEngine, name, None)), name
    for cls in (runner.Runner, runner.Pool):
        assert callable(getattr(cls, "add_voice", None)), cls
    assert callable(getattr(runner.Runner, "list_voices", None))


def test_common_declares_add_voice_and_parler_runner_overrides_it():
    common = _read("tts.cpp_amd", "host", "common.h")
    assert re.search(r"virtual\s+void\s+add_voice\(const char \*\s*name,\s*const char \*\s*text_encoder_path,\s*const char \*\s*description\)\s*;", common)
    text = _read("tts.cpp_amd", "host", "parler_runner.h")
    assert re.search(r"void\s+add_voice\(const char \*\s*name,\s*const char \*\s*text_encoder_path,\s*const char \*\s*description\)\s*override;", text)
    assert re.search(r"list_voices\(\)\s*override;", text)
    for stale in ("the voice description stays the session's", "The voice description stays the session's"):
        assert stale not in common and stale not in text, stale
    assert "One voice description per session stays" not in _read("DESIGN.md")


def test_add_voice_is_the_last_virtual_of_the_runner_class():
    """an application compiled against the earlier common.h (the reference's cli, perf_battery and server through compat/) calls generate(),
    list_voices() and update_conditional_prompt() by their place in the class: the new virtual comes after every virtual that was there"""
    common = _read("tts.cpp_amd", "host", "common.h")
    cls = common[common.index("struct tts_generation_runner : tts_runner {"):]
    cls = cls[:cls.index("\n};")]
    virtuals = re.findall(r"^\s*virtual\s+[\w:<> ]+?[\s*&]+(\w+)\(", cls, flags=re.M)
    assert virtuals[-1] == "add_voice" and virtuals.count("add_voice") == 1, virtuals
    assert {"generate", "list_voices", "update_conditional_prompt", "generate_batch", "stream_accepts", "generate_batch_chunked"} <= set(virtuals[:-1])


def test_a_runner_without_voice_descriptions_refuses_add_voice():
    r = runner.Runner("test:dummy")
    with pytest.raises(runner.RunnerError, match="no voice descriptions"):
        r.add_voice("a", "/nonexistent/t5.gguf", "a calm voice")
    assert r.generate("ab").size == 2 * 44100       # ... and goes on
    r.close()
    pool = runner.Pool("test:dummy", n_workers=2, max_batch=2, text_encoder_path="/nonexistent/t5.gguf")
    audio, bs, wk, err = pool.wait(pool.add_voice("a", "a calm voice"), 20000)
    assert audio.size == 0 and "no voice descriptions" in err
    audio, bs, wk, err = pool.wait(pool.submit("ab"), 20000)
    assert err == "" and audio.size == 2 * 44100
    pool.close()
    pool = runner.Pool("test:dummy", n_workers=1, max_batch=2)   # no text encoder: the message of CONDITIONAL_PROMPT
    audio, bs, wk, err = pool.wait(pool.add_voice("a", "a calm voice"), 20000)
    assert audio.size == 0 and "text encoder path" in err
    pool.close()


def test_the_dummy_session_still_refuses_a_differing_voice():
    """stream_accepts of a runner without the extension stays false: a request that differs in its voice alone does not join the open session
    (it is served by a session of its own), and generate_stream with per-sentence voices runs them as consecutive sessions with unchanged audio"""
    r = runner.Runner("test:dummy")
    texts = ["ab", "c", "de"]
    got = r.generate_stream(texts, configs=[dict(voice=""), dict(voice="x"), dict(voice="")])
    for t, a in zip(texts, got):
        assert a.size == len(t) * 44100
    r.close()
    pool = runner.Pool("test:dummy", n_workers=1, max_batch=4, continuous=True, continuous_yield_ms=50)
    first = pool.submit("a" * 10)                   # ten look-in intervals of generation
    other = pool.submit("zz", voice="x")            # queued behind it: the open session is asked and refuses
    for i in (first, other):
        audio, bs, wk, err = pool.wait(i, 20000)
        assert err == "" and audio.size > 0
    st = pool.stats()
    assert st["batches"] == 2 and st["admitted_in_flight"] == 0, st
    pool.close()
