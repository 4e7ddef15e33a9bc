"""afg_mp3_requant_hip on hand-made records (tests/mp3_requant_cases.py): the arithmetic switch points, tables, stereo plans
and plane layouts that the file-driven tests of tests/test_mp3_requant_gpu.py reach rarely or never, bit for bit against
the float32 model (tests/mp3_requant_model.py) and word for word against a sentinel everywhere the launch must not write.

What the file-driven inputs reach: cases.branches summed over the 19 files of test_mp3_requant_gpu.files() (366 granule
records, 210 816 lines), beside one hand-made launch, cases.hand_made(5) (200 records, 190 080 lines).  Lines per class;
records for nch and offsets_differ:

    class                          files()   hand_made(5)
    zero                           324 530       61 984
    table (|v| 1 .. 128)            54 659       67 571
    formula, |v| below 1024            703       30 197
    formula, |v| from 1024 up          268       30 328
    sign step taken, below 1024        427       15 035
    sign step not taken, below 1024    276       15 162
    sign step taken, from 1024 up       95       14 425
    sign step not taken, from 1024     173       15 903
    |v| = 8206                          33          661
    stereo mode 0 / 1 / 2 per line  29 884 / 94 052 / 45 408     38 524 / 38 300 / 9 576
    both lines zero under mid/side  64 225        4 064
    zero line under intensity       42 408        3 168
    fl 0 / 1 / negative             10 546 / 10 102 / 0          3 238 / 1 656 / 2 434
    fr 0 / 1 / negative                438 / 10 114 / 0          2 412 / 2 174 / 2 444
    channel 0 reordered yes / no    57 024 / 153 792            60 480 / 43 200
    channel 1 reordered yes / no    33 408 / 135 936            48 384 / 38 016
    t0 != t1                        64 512       73 152
    reorder bits differ             57 024       36 864
    q_off != coef_off (records)          0          180
    nch 0 / 1 / 2 (records)              0 / 72 / 294               20 / 30 / 150

The files never have a negative intensity factor, an unused slot or q_off != coef_off; 0.5 % of their lines take
L3_pow_43's formula.  Of the 24 band tables they use 18 as table[0] and 15 as table[1]: rows 1 and 2 (MPEG-2.5 at 8 kHz,
MPEG-2 at 22.05 kHz) of no kind, and row 7 never for the right channel; their two channels always share the rate row."""
import numpy as np
import pytest

import afgpu
import mp3_bitstream as mb
import mp3_requant_cases as cases

pytestmark = pytest.mark.gpu


def launch(gpu, q, gr, sd, coef_floats):
    """one launch over a plane of SENTINEL words; the plane's words afterwards"""
    import torch
    assert int((gr["q_off"] + 576 * gr["nch"].astype(np.uint64)).max()) <= q.size
    assert int((gr["coef_off"] + 576 * gr["nch"].astype(np.uint64)).max()) <= coef_floats
    assert not len(sd) or int(gr["sdesc"][gr["stereo"] == 2].max(initial=0)) < len(sd)
    d_q = torch.from_numpy(q.reshape(-1).copy()).to(gpu)
    d_gr = torch.from_numpy(np.ascontiguousarray(gr).view(np.uint8).copy()).to(gpu)
    d_sd = torch.from_numpy(np.ascontiguousarray(sd).view(np.uint8).copy()).to(gpu) if len(sd) else None
    d_coef = torch.from_numpy(np.full(coef_floats, cases.SENTINEL, np.uint32).view(np.int32)).to(gpu)
    afgpu.mp3_requant(len(gr), d_gr, d_q, d_sd, d_coef.view(torch.float32))
    torch.cuda.synchronize()
    return d_coef.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("seed", [5, 6])
def test_hand_made_records(gpu, seed):
    """every float of a granule equals the model's bit for bit; every other float of the plane still holds the sentinel:
    the gaps, the block an unused slot points at, the block behind a mono granule"""
    q, gr, sd, coef_floats, mask = cases.hand_made(seed)
    want = cases.expected_hand_made(seed)
    got = launch(gpu, q, gr, sd, coef_floats)
    cases.same_words(got, want, q, gr, sd)
    assert (got[~mask] == cases.SENTINEL).all() and (got[mask] != cases.SENTINEL).all()


@pytest.mark.parametrize("seed", [5, 6])
def test_records_in_another_order_give_the_same_plane(gpu, seed):
    """the records reversed, and behind one more unused slot: the same blocks get the same bits wherever their record
    stands in the launch (the record index reaches nothing but the record; the bound on it holds the last one)"""
    q, gr, sd, coef_floats, mask = cases.hand_made(seed)
    want = cases.expected_hand_made(seed)
    cases.same_words(launch(gpu, q, gr[::-1].copy(), sd, coef_floats), want, q, gr, sd)
    slot = gr[gr["nch"] == 0][:1].copy()
    cases.same_words(launch(gpu, q, np.concatenate([slot, gr]), sd, coef_floats), want, q, gr, sd)


@pytest.mark.parametrize("nch", [0, 1, 2])
def test_a_single_granule(gpu, nch):
    q, gr, sd, coef_floats, mask = cases.hand_made(5)
    for stereo in ((0, 1, 2) if nch == 2 else (0,)):
        one = gr[(gr["nch"] == nch) & (gr["stereo"] == stereo)][:1].copy()
        assert len(one) == 1
        want = cases.expected(q, one, sd, coef_floats)
        assert int((want != cases.SENTINEL).sum()) == 576 * nch
        cases.same_words(launch(gpu, q, one, sd, coef_floats), want, q, one, sd)


@pytest.mark.parametrize("kw", [dict(version="mpeg1", sr=0, mode="stereo"), dict(version="mpeg1", sr=1, mode="ms"),
                                dict(version="mpeg2", sr=2, mode="ms+intensity"), dict(version="mpeg1", sr=2, mode="mono")],
                         ids=lambda kw: kw["mode"])
def test_records_of_a_file_moved_about_the_planes(gpu, kw):
    """ties the hand-made model to the chain the suite already trusts: the records afg_mp3_parse_q makes of a generated file,
    moved into shuffled, gapped planes with q_off != coef_off, give the spectra of afgpu.mp3_parse -- the float front-end
    the oracle pins -- block by block, and nothing else is written"""
    data = mb.make_file(91, n_frames=12, **kw)[0]
    info, runs, q, flags, copies, gr, sd = afgpu.mp3_parse_q(data)
    coef = afgpu.mp3_parse(data)[2]
    assert len(gr) and (gr["stereo"] == {"stereo": 0, "ms": 1, "ms+intensity": 2, "mono": 0}[kw["mode"]]).all()
    plane, moved, coef_floats, src = cases.rebased(np.random.default_rng(7), q, gr)
    want = np.full(coef_floats, cases.SENTINEL, np.uint32)
    for g, s in zip(moved, src):
        n = 576 * int(g["nch"])
        want[int(g["coef_off"]):int(g["coef_off"]) + n] = coef[int(s):int(s) + int(g["nch"])].reshape(-1).view(np.uint32)
    cases.same_words(launch(gpu, plane, moved, sd, coef_floats), want, plane, moved, sd)
