"""Holds the two CPU statements of the QOA frame decoder to each other, bit for bit: the integer model (qoa_model.py, NumPy
int64 with the 32-bit wraps written out) and the oracle (oracle/qoa_lms.c, C unsigned arithmetic).  The oracle is
otherwise pinned on encoder output only (test_oracle_qoa.py), where nothing wraps; here the inputs are arbitrary slice
words and LMS state: every case tests/test_qoa_decode_edges_gpu.py launches (qoa_cases.gpu_cases), the frames
tests/test_qoa_gpu.py crafts (qoa_cases.crafted_cases: 5120, 12000 and 20000 samples at the largest scalefactor), real
files, and four steps worked out by hand."""
import numpy as np
import pytest

import afgpu
import oraclelib
import qoa_cases
import qoa_model
from test_oracle_qoa import tone


def agree(frames, data, out_total):
    """model == oracle in every value a frame writes, int16 and float bits; the oracle writes nothing else"""
    written, mi, mf = qoa_model.decode(frames, data, out_total)
    oi, of = oraclelib.qoa_transform(frames, data, out_total)
    assert int(written.sum()) == int((frames["samples"].astype(np.int64) * frames["channels"]).sum())
    assert (oi[written] == mi[written]).all()
    assert (of[written].view(np.uint32) == mf[written].view(np.uint32)).all()
    assert not oi[~written].any() and not of[~written].view(np.uint32).any()
    return mi


def case_agrees(case):
    written, mi, mf = case.model()
    oi, of = case.oracle()
    assert (oi[written] == mi[written]).all(), case.name
    assert (of[written].view(np.uint32) == mf[written].view(np.uint32)).all(), case.name
    assert not oi[~written].any() and not of[~written].view(np.uint32).any(), case.name


def test_four_steps_by_hand():
    """One mono frame of four samples, scalefactor 0, codes 0 1 2 7 (+1 -1 +3 -7), from the encoder's start state: zero
    history, weights {0, 0, -8192, 16384} (test_oracle_qoa.py::test_first_samples_by_hand).
      1: p = 0;                                     v = 1;  delta = 1 >> 4 = 0
      2: p = 16384 * 1 >> 13 = 2;                   v = 1;  delta = -1 >> 4 = -1, no history negative: every weight - 1
      3: p = (-8193 + 16383) >> 13 = 0;             v = 3;  delta = 0
      4: p = (-1 - 8193 + 3 * 16383) >> 13 = 4;     v = -3; delta = -7 >> 4 = -1"""
    frames = np.zeros(1, afgpu.QOA_FRAME_DTYPE)
    frames[0] = (8, 3, 4, 1, 0)
    words = [0, (1 << 56) | (44100 << 32) | (4 << 16) | (8 + 16 + 8), 0, (0xE000 << 16) | 0x4000, (0b000001010111 << 48)]
    data = np.array(words, ">u8").view(np.uint8)
    stats = {}
    written, mi, mf = qoa_model.decode(frames, data, 9, stats)
    assert list(mi) == [0, 0, 0, 1, 1, 3, -3, 0, 0] and list(written) == [False] * 3 + [True] * 4 + [False] * 2
    assert (mf.view(np.uint32) == (mi.astype(np.float32) * np.float32(1.0 / 32767)).view(np.uint32)).all()
    assert stats["max_abs_weight"][0] == 16384
    assert list(oraclelib.qoa_transform(frames, data, 9, want_float=False)) == list(mi)
    # the weights after the four steps, read off the next prediction: history 1 1 3 -3, weights -2 -2 -8194 16382
    h = np.array([[0, 0, 0, 0]], np.int64)
    w = np.array([[0, 0, -8192, 16384]], np.int64)
    for deq in (1, -1, 3, -7):
        qoa_model.step(h, w, np.array([deq], np.int64))
    assert h.tolist() == [[1, 1, 3, -3]] and w.tolist() == [[-2, -2, -8194, 16382]]


def test_wrap32():
    v = np.array([0, 1, -1, 2**31 - 1, 2**31, -2**31, -2**31 - 1, 2**32, 3 * 2**32 + 5, -(2**47) + 7], np.int64)
    assert qoa_model.wrap32(v).tolist() == [0, 1, -1, 2**31 - 1, -2**31, -2**31, 2**31 - 1, 0, 5, 7]


def test_silence_file():
    """the file of test_oracle_qoa.py::test_first_samples_by_hand: both decoders return the encoder's reconstruction"""
    data, recon = oraclelib.qoa_encode(np.zeros((40, 1), np.int16))
    frames, *_ = afgpu.qoa_frames(data.tobytes())
    assert (agree(frames, data, 40) == recon.reshape(-1)).all()


@pytest.mark.parametrize("n,ch", [(5120 * 2 + 777, 2), (5120, 1), (19, 2), (12345, 3), (41, 8)])
def test_encoded_files(n, ch):
    pcm = tone(n, ch, seed=n)
    data, recon = oraclelib.qoa_encode(pcm)
    frames, *_ = afgpu.qoa_frames(data.tobytes())
    assert (agree(frames, data, n * ch).reshape(n, ch) == recon).all()


def test_encoded_file_with_random_state_and_slices():
    """tests/test_qoa_gpu.py::test_qoa_wrapping_lms_state's input"""
    rng = np.random.default_rng(3)
    data, _ = oraclelib.qoa_encode(tone(5120 * 2, 2, seed=1))
    frames, *_ = afgpu.qoa_frames(data.tobytes())
    for fr in frames:
        b = int(fr["byte_off"])
        data[b + 8:b + 40] = rng.integers(0, 256, 32, dtype=np.uint8)
        data[b + 40:b + 40 + 8 * 256 * 2] = rng.integers(0, 256, 8 * 256 * 2, dtype=np.uint8)
    agree(frames, data, 5120 * 2 * 2)


GPU_CASES, CRAFTED_CASES = qoa_cases.gpu_cases(), qoa_cases.crafted_cases()


@pytest.mark.parametrize("make", [m for _, m in GPU_CASES], ids=[n for n, _ in GPU_CASES])
def test_gpu_cases(make):
    case_agrees(make())


@pytest.mark.parametrize("make", [m for _, m in CRAFTED_CASES], ids=[n for n, _ in CRAFTED_CASES])
def test_crafted_cases(make):
    case_agrees(make())


def test_the_cases_reach_what_they_are_for():
    """Random slices, all-ones slices, extreme state and every frame length are among the cases; the driven frames
    (qoa_cases.driven_words) take a weight 896 per sample beyond the int16 it starts from -- to the edge of 24 bits in 9000
    samples and past it in 9400 -- where a repeated word leaves the weights below 2^18 (the prediction wraps and the
    history's signs turn random)."""
    names = [n for n, _ in GPU_CASES + CRAFTED_CASES]
    for part in ("odd_tails", "general", "switch9000-", "switch9020-", "switch9020+short-", "crafted12000-random", "crafted12000-ones",
                 "crafted20000-half", "crafted20000-ones", "crafted5120-ffffffffffffffff-1", "zero_records"):
        assert any(n.startswith(part) for n in names), part
    for kind, least in (("9000", 32767 + 8900 * 896), ("9020", 32767 + 8900 * 896), ("9400", 1 << 23)):
        case = qoa_cases.switch(kind, "driven")
        case.model()
        assert (case.peak > least).all(), kind
    for kind in ("9000", "9020", "9400"):
        for word in qoa_cases.LARGEST_WORDS:
            case = qoa_cases.switch(kind, word)
            case.model()
            assert (case.peak < 1 << 18).all(), (kind, word)
