"""Host logic of maed_amd/video.py: windows, reflect padding and the chunking rule, checked on the index tables alone (no GPU, no kernels, no pixels)."""
import numpy as np
import pytest

from maed_amd import video as V


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33])
def test_windows_pad_like_numpy_reflect(n):
    """lib/data_utils/img_utils.py:32-54 with pad=True: np.pad(indices, (0, padlen), 'reflect') -- the edge sample is not repeated, a single index repeats"""
    seqlen = 16
    pos, real = V.window_positions(n, seqlen)
    padlen = (seqlen - n % seqlen) % seqlen
    want = np.pad(np.arange(n), (0, padlen), "reflect")
    assert pos.shape == real.shape == (len(want) // seqlen, seqlen)
    assert np.array_equal(pos.reshape(-1), want)
    assert np.array_equal(real.reshape(-1), np.arange(len(want)) < n)          # the padded slots trail, and only they are marked
    assert pos.min() >= 0 and pos.max() == n - 1


def test_reflect_does_not_repeat_the_edge():
    assert V.window_positions(3, 8)[0].tolist() == [[0, 1, 2, 1, 0, 1, 2, 1]]
    assert V.window_positions(1, 4)[0].tolist() == [[0, 0, 0, 0]]


def _check_plan(chunks, people, seqlen, frame_bytes, clips_per_batch, max_crops=V.MAX_CROPS):
    seen = {}
    for c in chunks:
        M = len(c["box_index"])
        assert M == len(c["frame_index"]) == len(c["windows"]) * seqlen and len(c["windows"]) <= clips_per_batch and M <= max_crops
        assert c["frame_index"].dtype == np.int32 and c["box_index"].dtype == np.int32
        assert c["frame_index"].min() >= 0 and c["frame_index"].max() < c["n_frames"]
        # what maed_crop_tables writes into frame_i[:, 0], and the last byte a tap may touch, in exact integers
        off = c["frame_index"].astype(object) * frame_bytes
        assert max(off) + frame_bytes <= c["n_frames"] * frame_bytes < 2 ** 31
        for n, (pi, wi, real_n) in enumerate(c["windows"]):
            assert (pi, wi) not in seen
            seen[(pi, wi)] = (c["first_frame"] + c["frame_index"][n * seqlen:(n + 1) * seqlen], c["box_index"][n * seqlen:(n + 1) * seqlen], real_n)
    for pi, (frame_ids, base) in enumerate(people):
        pos, real = V.window_positions(len(frame_ids), seqlen)
        for wi in range(len(pos)):
            f, b, real_n = seen.pop((pi, wi))
            assert np.array_equal(f, np.asarray(frame_ids)[pos[wi]]) and np.array_equal(b, base + pos[wi]) and real_n == real[wi].sum()
    assert not seen


def test_chunks_keep_every_table_offset_below_2_31():
    """a DECLARED frame size of 2160 x 3840 and 400 frames (9.9 GB of pixels that are never allocated): at most 86 frames fit below 2^31 bytes"""
    frame_bytes = 2160 * 3840 * 3
    rng = np.random.default_rng(1)
    people = [(np.arange(400), 0), (np.arange(37, 290), 1000), (np.sort(rng.choice(400, 120, replace=False))[:60], 5000), (np.array([399]), 7000)]
    chunks = V.plan_chunks(people, 16, frame_bytes, 8)
    _check_plan(chunks, people, 16, frame_bytes, 8)
    assert max(c["n_frames"] for c in chunks) <= 86 and len(chunks) > 400 // 86
    # small frames: the same people in chunks of clips_per_batch windows
    chunks = V.plan_chunks(people, 16, 96 * 128 * 3, 8)
    _check_plan(chunks, people, 16, 96 * 128 * 3, 8)
    assert sorted(len(c["windows"]) for c in chunks)[1:] == [8] * (len(chunks) - 1)


def test_chunks_keep_to_the_crop_bound():
    people = [(np.arange(100), 0)]
    chunks = V.plan_chunks(people, 16, 300, 1000, max_crops=40)       # 40 crops per call: two windows of 16
    _check_plan(chunks, people, 16, 300, 1000, max_crops=40)
    assert max(len(c["windows"]) for c in chunks) == 2
    with pytest.raises(ValueError, match="crops"):
        V.plan_chunks(people, 16, 300, 4, max_crops=8)


def test_a_window_that_cannot_be_addressed_is_refused():
    """out of scope by design: one window whose frames span 2^31 bytes or more"""
    with pytest.raises(ValueError, match=r"2\^31"):
        V.plan_chunks([(np.array([0, 399]), 0)], 16, 2160 * 3840 * 3, 8)
    with pytest.raises(ValueError, match="65535"):
        V.VideoInference(None, seqlen=70000)
