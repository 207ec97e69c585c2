"""Per-request configurations in a continuous session, the parts that need no device: the new C symbols, the two virtuals of
tts_generation_runner, generate_stream with one configuration per sentence on the weightless dummy runner (whose stream_accepts is false),
and the pool's yield rule, which must not move."""
import ctypes
import os
import re
import time

import numpy as np

from tts_cpp_amd import hip, runner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_NEW = ["tts_hip_orpheus_stream_begin_mixed", "tts_hip_orpheus_stream_admit_mixed", "tts_hip_orpheus_sample_logits_rows_mixed"]
C_NEW = ["tts_c_generate_stream_configs"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_new_symbols_are_declared_listed_and_exported():
    for names, header, exports, lib in ((HIP_NEW, "tts_hip.h", hip.EXPORTS, os.path.join(ROOT, "tts.cpp_amd", "libtts_hip.so")),
                                        (C_NEW, "tts_c.h", runner.EXPORTS, runner.lib_path())):
        text = _read("include", header)
        L = ctypes.CDLL(lib)
        for name in names:
            assert re.search(r"\b" + name + r"\s*\(", text), (header, name)
            assert name in exports, name
            assert hasattr(L, name), (lib, name)


def test_common_h_declares_the_two_virtuals():
    text = _read("tts.cpp_amd", "host", "common.h")
    assert re.search(r"virtual\s+bool\s+stream_accepts\(const generation_configuration &\s*\w*\)\s*const", text)
    assert re.search(r"virtual\s+void\s+stream_submit\(size_t \w+, const std::string &\s*\w+, const generation_configuration &\s*\w*\)", text)


def test_generate_stream_with_per_sentence_configs_on_the_dummy_runner():
    """the dummy accepts nothing beside its session's configuration: the sentences run as consecutive sessions of equal configurations, and every
    utterance comes back with the audio of its own generate() call (one second per character)"""
    r = runner.Runner("test:dummy")
    texts = ["ab", "c", "def", "g", "hi", "j", "klm"]
    cfgs = [dict(top_k=7), dict(top_k=7), dict(top_k=9), dict(top_k=9, temperature=0.5), dict(top_k=7), dict(top_k=7), dict(top_k=7)]
    got = r.generate_stream(texts, configs=cfgs)
    assert len(got) == len(texts)
    for t, a in zip(texts, got):
        assert a.size == len(t) * 44100 and np.array_equal(a, r.generate(t))
    assert r.generate_stream([], configs=[]) == []
    r.close()


def test_pool_over_the_dummy_still_yields_to_an_incompatible_request():
    """the dummy's stream_accepts is false, so a request with other sampling parameters is still left behind by a running session, and once it has
    waited continuous_yield_ms the session drains for it: it comes back before the compatible requests submitted behind it have all been served"""
    pool = runner.Pool("test:dummy", n_workers=1, max_batch=4, continuous=True, continuous_yield_ms=50)
    first = [pool.submit("a" * 10) for _ in range(2)]           # 0.1 s of generation each
    time.sleep(0.02)
    other = pool.submit("zz", top_k=7)                          # incompatible with the running session
    later = []
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.3:                       # a steady stream of compatible requests
        later.append(pool.submit("b" * 5))
        time.sleep(0.01)
    audio, bs, wk, err = pool.wait(other, 20000)
    t_other = time.perf_counter() - t0
    assert err == "" and audio.size == 2 * 44100
    assert all(pool.wait(i, 20000)[3] == "" for i in later)
    t_all = time.perf_counter() - t0
    assert t_other < t_all - 0.05, (t_other, t_all)             # served before the stream behind it had drained
    assert pool.stats()["batches"] >= 3                         # the session ended for it, and another one followed
    for i in first:
        pool.wait(i, 20000)
    pool.close()
