"""Host side of the Kokoro duration groups (TTS_KOKORO_ROWS), without a device: the new symbol is declared, listed and exported, and the two pure functions
generate_batch plans with (host/kokoro_runner.h) hold their contracts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tts_cpp_amd import hip, runner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_call_is_declared_listed_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tts_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+tts_hip_kokoro_durations_batch\s*\(\s*tts_hip_ctx\s*\*", hdr)
    assert re.search(r"#define\s+TTS_HIP_KOKORO_ROWS_MAX\s+8\b", hdr)
    assert "tts_hip_kokoro_durations_batch" in hip.EXPORTS
    assert os.path.exists(hip.lib_path()), "libtts_hip.so not built (run __graft_entry__.build())"
    assert hasattr(C.CDLL(hip.lib_path()), "tts_hip_kokoro_durations_batch")
    L = C.CDLL(runner.lib_path())
    for name in ("tts_c_kokoro_duration_groups", "tts_c_kokoro_noise_starts"):
        assert name in runner.EXPORTS and hasattr(L, name), name
    assert b"tts_hip_kokoro_durations_batch" in open(runner.lib_path(), "rb").read()   # generate_batch calls it


def check_plan(lengths, cap):
    groups = runner.kokoro_duration_groups(lengths, cap)
    flat = [i for g in groups for i in g]
    assert sorted(flat) == list(range(len(lengths)))                       # every piece in exactly one group
    assert all(1 <= len(g) <= cap for g in groups)
    assert all(len(g) == cap for g in groups[:-1])                         # consecutive runs: only the last may be short
    lens = [lengths[i] for i in flat]
    assert all(a >= b for a, b in zip(lens, lens[1:]))                     # non-increasing inside and across groups
    assert all(i < j for i, j, a, b in zip(flat, flat[1:], lens, lens[1:]) if a == b)   # equal lengths keep the input order
    assert runner.kokoro_duration_groups(lengths, cap) == groups          # the same input, the same plan
    return groups


def test_duration_groups_by_hand():
    assert check_plan([5, 34, 3, 32, 31, 33, 5, 4], 8) == [[1, 5, 3, 4, 0, 6, 7, 2]]
    assert check_plan([5, 34, 3, 32, 31, 33, 5, 4], 3) == [[1, 5, 3], [4, 0, 6], [7, 2]]
    assert check_plan([7, 7, 7], 2) == [[0, 1], [2]]
    assert check_plan([400] * 11, 8) == [list(range(8)), [8, 9, 10]]
    assert check_plan([3], 8) == [[0]]
    assert check_plan([3, 512], 1) == [[1], [0]]
    assert runner.kokoro_duration_groups([], 8) == []
    with pytest.raises(runner.RunnerError):
        runner.kokoro_duration_groups([3, 4], 0)


def test_duration_groups_on_random_lists():
    rng = np.random.default_rng(8)
    for _ in range(200):
        n = int(rng.integers(1, 41))
        # few distinct values in half of the lists, so that ties are common
        lengths = rng.integers(3, 513, n) if rng.random() < 0.5 else rng.choice([3, 4, 66, 402, 512], n)
        check_plan([int(v) for v in lengths], int(rng.integers(1, 9)))


def test_noise_starts_are_the_chain_of_jumps():
    L = runner.load_lib()
    L.tts_c_minstd0_jump.restype = C.c_uint32
    L.tts_c_minstd0_jump.argtypes = [C.c_uint32, C.c_uint64]
    rng = np.random.default_rng(9)
    for per_frame in (1, 9, 5400):
        for n in (0, 1, 2, 11, 40):
            frames = rng.integers(0, 20000, n)
            if n > 2:
                frames[[0, n // 2]] = 0                                    # zero-frame pieces: the next piece starts at the same state
            state = int(rng.integers(1, 2**31 - 1))
            starts, end = runner.kokoro_noise_starts(state, frames, per_frame)
            assert starts.size == n
            for i in range(n):
                assert int(starts[i]) == state, (per_frame, n, i)
                state = int(L.tts_c_minstd0_jump(state, int(frames[i]) * per_frame))
            assert end == state
    # far past 2^32 draws in one piece
    starts, end = runner.kokoro_noise_starts(1, [2**33, 1], 5400)
    assert int(starts[1]) == int(L.tts_c_minstd0_jump(1, 2**33 * 5400)) and end == int(L.tts_c_minstd0_jump(int(starts[1]), 5400))
