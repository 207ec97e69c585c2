"""The chunk-window planner of the Parler and Dia runners (host/chunk_windows.h through tts_c_chunk_windows), without a device: a delayed token
stream is fed to the planner piece by piece and then once more marked finished, and the windows it cuts are checked against the un-delay
rules' own output (tts_c_parler_final_frames, tts_c_dia_final_frames)."""
import numpy as np
import pytest

from tts_cpp_amd import hip, runner, synth

DIA_MAX_DELAY = 15
AUDIO_VOCAB = 64
DAC44K_HALO = hip.dac_halo_frames(hip.desc_for(synth.parler_mini()))   # as tests/test_chunked_cpu.py obtains it: 10
HALOS = (0, 1, DAC44K_HALO)
CHUNKS = (1, 8, 10 ** 6)          # the last: more than any stream here holds
PIECES = (1, 16, 32, 0)           # 0: the whole stream at once


def _stream(rule, halo, chunk_frames, dropped, seed=0):
    """about 3 halos + 3 chunks + the delay steps of random audio ids [steps][heads]; `dropped`: ids outside the audio vocabulary mid-stream, each
    of which takes its frame out of the kept sequence"""
    rng = np.random.default_rng(seed)
    nh, delay = (4, 3) if rule == "parler" else (9, DIA_MAX_DELAY)
    steps = 3 * halo + 3 * min(chunk_frames, 8) + delay + 5
    t = rng.integers(0, AUDIO_VOCAB, (steps, nh)).astype(np.uint32)
    if dropped:
        for s in (4, steps // 2, steps // 2 + 1, steps - delay - 2):
            t[s, rng.integers(0, nh)] = AUDIO_VOCAB + rng.integers(0, 3)
    return t


def _final_frames(rule, toks, finished):
    """the kept frames that are final after these steps, by the rule's own entry point"""
    if rule == "parler":
        return runner.parler_final_frames(toks, AUDIO_VOCAB, finished)
    return runner.dia_final_frames(toks, AUDIO_VOCAB, DIA_MAX_DELAY)   # Dia's rule has no end-of-stream case: the last max_delay steps judge nothing


def _plan(rule, toks, halo, chunk_frames, piece):
    return runner.chunk_windows(rule, toks, AUDIO_VOCAB, halo, chunk_frames, piece, max_delay=DIA_MAX_DELAY)


def _check(rule, toks, halo, chunk_frames, piece):
    """every property of one plan -> the concatenation of its kept frames"""
    nh = toks.shape[1]
    win, cut, codes = _plan(rule, toks, halo, chunk_frames, piece)
    full = _final_frames(rule, toks, True).reshape(-1, nh)
    have = len(full)
    tag = (rule, halo, chunk_frames, piece)
    assert codes.shape == full.shape and np.array_equal(codes, full), tag          # frames [0, have), nothing else
    emitted = 0
    for i, ((w0, w1, k0, k1), (steps, finished)) in enumerate(zip(win.tolist(), cut.tolist())):
        first, last = w0 + k0, w0 + k1 - 1                                          # the kept frames, counted in the utterance
        assert first == emitted and last >= first, (tag, i)                         # without gap or overlap, and never empty
        final = len(_final_frames(rule, toks[:steps], bool(finished)))              # frames final when it was cut
        assert w0 == max(0, first - halo) and w1 == min(final, last + 1 + halo), (tag, i)
        if not finished:
            assert last + 1 + halo <= final, (tag, i, "cut before its right halo was final")
            assert (last + 1 - first) % chunk_frames == 0, (tag, i)
        else:
            assert i == len(win) - 1 and steps == len(toks), (tag, i)               # only the last window may hold a part of a chunk
        emitted = last + 1
    assert emitted == have, tag
    if have == 0:
        assert len(win) == 0, tag
    return codes


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("rule", ["parler", "dia"])
def test_windows_tile_the_final_frames(rule, halo, dropped):
    for chunk_frames in CHUNKS:
        toks = _stream(rule, halo, chunk_frames, dropped)
        if dropped:
            assert len(_final_frames(rule, toks, True)) < len(_final_frames(rule, _stream(rule, halo, chunk_frames, False), True)), "frames must be dropped"
        cats = [_check(rule, toks, halo, chunk_frames, piece) for piece in PIECES]
        for c in cats[1:]:
            assert np.array_equal(c, cats[0]), "the concatenation does not depend on the piece size"


@pytest.mark.parametrize("halo", HALOS)
def test_unfinished_streams_cut_whole_chunks_only(halo):
    """a window cut while the stream runs holds whole chunks whose right halo is final; with chunk_frames 8 and pieces of 1 step every such
    window is exactly one chunk, cut at the first step at which frame (last kept + halo) is final"""
    for rule in ("parler", "dia"):
        toks = _stream(rule, halo, 8, False)
        win, cut, _ = _plan(rule, toks, halo, 8, 1)
        running = [(w, c) for w, c in zip(win.tolist(), cut.tolist()) if not c[1]]
        assert len(running) >= 3, (rule, halo)
        for (w0, w1, k0, k1), (steps, _) in running:
            assert k1 - k0 == 8
            assert len(_final_frames(rule, toks[:steps], False)) == w0 + k1 + halo          # just enough ...
            assert len(_final_frames(rule, toks[:steps - 1], False)) == w0 + k1 + halo - 1  # ... and not a step earlier


def test_nothing_kept_yields_no_window():
    rng = np.random.default_rng(3)
    for rule, nh in (("parler", 4), ("dia", 9)):
        bad = np.full((40, nh), AUDIO_VOCAB, dtype=np.uint32)                       # every frame holds a non-audio id
        for piece in PIECES:
            win, cut, codes = _plan(rule, bad, 1, 8, piece)
            assert len(win) == 0 and len(cut) == 0 and len(codes) == 0, (rule, piece)
        win, _, codes = _plan(rule, bad[:0], 1, 8, 0)                               # no steps at all
        assert len(win) == 0 and len(codes) == 0
    for steps in range(0, DIA_MAX_DELAY + 1):                                       # a Dia stream shorter than max_delay judges no frame
        toks = rng.integers(0, AUDIO_VOCAB, (steps, 9)).astype(np.uint32)
        for piece in PIECES:
            assert len(_plan("dia", toks, DAC44K_HALO, 8, piece)[0]) == 0, (steps, piece)
    toks = rng.integers(0, AUDIO_VOCAB, (DIA_MAX_DELAY + 1, 9)).astype(np.uint32)   # one step more: one frame, one window at the end
    win, cut, codes = _plan("dia", toks, DAC44K_HALO, 8, 1)
    assert win.tolist() == [[0, 1, 0, 1]] and cut.tolist() == [[DIA_MAX_DELAY + 1, 1]] and len(codes) == 1


def test_bad_arguments_are_refused():
    toks = np.zeros((4, 4), dtype=np.uint32)
    with pytest.raises(runner.RunnerError, match="tts_c_chunk_windows"):
        runner.chunk_windows("parler", toks, AUDIO_VOCAB, 1, 0)
    assert "tts_c_chunk_windows" in runner.EXPORTS
