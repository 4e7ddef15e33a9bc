"""afg_filter_hip on the device against tests/filter_model.py: every output inside the interval of include/afg.h round the
model's long-double sequential result, with K from the header; in place against out of place and one row at two places bit
for bit; rows filtered in pieces through d_state; a NaN that spoils nothing in front of it or beside it."""
import functools
import math

import numpy as np
import pytest

import afgpu
import filter_model as fm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

T = afgpu.lib().afg_filter_tile_frames()
C16 = afgpu.FILTER_CHUNK
W = 64 * C16
K = afgpu.FILTER_K
LENGTHS = [0, 1, 2, 3, C16 - 1, C16, C16 + 1, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 1, 5 * T + C16 + 3]
KINDS = ("noise", "impulse", "ones")
SENTINEL = np.float32(1234.5)
CASCADES = {
    "preemphasis": [fm.design("preemphasis", f0=0.97)],
    "highpass_20": [fm.design("highpass", 48000.0, 20.0)],
    "voice": [fm.design("highpass", 16000.0, 80.0), fm.design("peaking", 16000.0, 1000.0, 2.0, 6.0), fm.design("lowpass", 16000.0, 7000.0)],
    "lowpass_near_nyquist": [fm.design("lowpass", 1.0, 0.45, 8.0)],
    # a sixteenth-order Butterworth low-pass at 0.1 fs: eight sections
    "eight_sections": [fm.design("lowpass", 1.0, 0.1, 1.0 / (2.0 * math.cos(math.pi * (2 * k + 1) / 32.0))) for k in range(8)],
}
LONG = 3 * LENGTHS.index(2 * T + 1)                             # the noise row of 2 T + 1 frames: the one that is cut and spoilt


@functools.lru_cache(maxsize=None)
def rows_in():
    """the launch's rows: every length with every kind of input, and two of the noise rows once more"""
    rng = np.random.default_rng(77)
    rows = []
    for n in LENGTHS:
        for kind in KINDS:
            x = np.zeros(n, np.float32)
            if kind == "noise":
                x[:] = rng.uniform(-1.0, 1.0, n).astype(np.float32)
            elif kind == "ones":
                x[:] = 1.0
            elif n:
                x[0] = 1.0
            rows.append(x)
    twins = [(3 * LENGTHS.index(T + 1), len(rows)), (3 * LENGTHS.index(5 * T + C16 + 3), len(rows) + 1)]
    rows += [rows[a].copy() for a, _ in twins]
    return rows, twins


@functools.lru_cache(maxsize=None)
def model(name):
    """(sig, E per row): the model's signals over the padded rows, computed once per cascade"""
    rows, _ = rows_in()
    X = np.zeros((len(rows), max(len(r) for r in rows)), np.float32)
    for k, r in enumerate(rows):
        X[k, :len(r)] = r
    sig = fm.run(CASCADES[name], X)
    E = fm.bound(CASCADES[name]) * np.array([np.abs(r).max() if len(r) else 0.0 for r in rows])
    return sig, E


def place(lengths, first, step):
    """float offsets of rows one after the other from `first`, 1 + (k * step) % 3 floats of sentinel between them; returns
    (offsets, floats of the plane)"""
    offs, at = [], first
    for k, n in enumerate(lengths):
        offs.append(at)
        at += n + 1 + (k * step) % 3
    return np.array(offs, np.uint64), at + 2


def launch(name, xs, in_place=False, state=None, first=(1, 3)):
    """the rows xs through one launch in sentinel-filled planes at odd offsets; returns the list of outputs, after checking
    that every float outside the rows is the sentinel still"""
    lengths = [len(x) for x in xs]
    in_off, in_floats = place(lengths, first[0], 1)
    out_off, out_floats = (in_off, in_floats) if in_place else place(lengths, first[1], 2)
    plane = np.full(in_floats, SENTINEL, np.float32)
    for o, x in zip(in_off, xs):
        plane[int(o):int(o) + len(x)] = x
    rec = np.zeros(len(xs), afgpu.FILTER_ROW_DTYPE)
    rec["in_off"], rec["out_off"], rec["frames"] = in_off, out_off, lengths
    d_in = torch.from_numpy(plane).cuda()
    d_out = d_in if in_place else torch.full((out_floats,), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_rows = torch.from_numpy(rec.view(np.uint8)).cuda()
    afgpu.filter_rows(len(xs), d_rows, CASCADES[name], d_in, in_floats, d_out, out_floats, state)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    outside = np.ones(out_floats, bool)
    for o, n in zip(out_off, lengths):
        outside[int(o):int(o) + n] = False
    assert (got[outside].view(np.uint32) == SENTINEL.view(np.uint32)).all(), "a float outside the rows was written"
    if not in_place:
        assert (d_in.cpu().numpy().view(np.uint32) == plane.view(np.uint32)).all(), "the input plane was written"
    return [got[int(o):int(o) + n].copy() for o, n in zip(out_off, lengths)]


def inside(got, want, KE, what):
    """every element of got inside the interval round want; returns the largest share of K E used"""
    if len(got) == 0:
        return 0.0
    err = np.abs(got.astype(fm.WIDE) - want).astype(np.float64)
    bad = np.flatnonzero(~(err <= fm.allowance(want, KE)))
    assert bad.size == 0, f"{what}: frame {bad[0]}: got {got[bad[0]]!r}, want {float(want[bad[0]])!r}, allowed {fm.allowance(want, KE)[bad[0]]!r}"
    return float(fm.share(got, want, KE).max())


@pytest.mark.parametrize("name", list(CASCADES))
def test_every_length_and_input_lies_inside_the_interval(name):
    rows, twins = rows_in()
    sig, E = model(name)
    out = launch(name, rows)
    used = 0.0
    for k, (x, y) in enumerate(zip(rows, out)):
        assert len(y) == len(x)
        used = max(used, inside(y, sig[-1][k, :len(x)], K * E[k], f"{name}: row {k} of {len(x)} frames") if len(x) else 0.0)
    print(f"filter {name}: {len(CASCADES[name])} sections, bound {fm.bound(CASCADES[name]):.3g}: largest share of K E used {used:.3g} (K = {K})")
    # the same row at two positions and alignments of the launch
    for a, b in twins:
        assert (out[a].view(np.uint32) == out[b].view(np.uint32)).all(), f"{name}: rows {a} and {b} differ"
    # in place
    same = launch(name, rows, in_place=True)
    for k, (y, z) in enumerate(zip(out, same)):
        assert (y.view(np.uint32) == z.view(np.uint32)).all(), f"{name}: row {k} differs in place"


@pytest.mark.parametrize("name", list(CASCADES))
def test_a_row_in_pieces_and_the_state_it_leaves(name):
    rows, _ = rows_in()
    sig, E = model(name)
    x, nsec = rows[LONG], len(CASCADES[name])
    KE = K * E[LONG]
    # the whole row: its outgoing state against the model's
    state = torch.zeros((1, nsec, 4), dtype=torch.float64, device="cuda")
    whole = launch(name, [x], state=state)[0]
    inside(whole, sig[-1][LONG, :len(x)], KE, f"{name}: the whole row")
    want = fm.state_at(sig, LONG, len(x))
    err = np.abs(state.cpu().numpy()[0].astype(fm.WIDE) - want).astype(np.float64)
    assert (err <= KE).all(), f"{name}: the state behind the row is off by {err.max()!r}, K E is {KE!r}"
    for cut in (T + 5, C16 - 1):
        state = torch.zeros((1, nsec, 4), dtype=torch.float64, device="cuda")
        head = launch(name, [x[:cut]], state=state)[0]
        mid = state.cpu().numpy()[0].astype(fm.WIDE)
        assert (np.abs(mid - fm.state_at(sig, LONG, cut)).astype(np.float64) <= KE).all(), f"{name}: the state at {cut}"
        tail = launch(name, [x[cut:]], state=state, first=(2, 1))[0]
        inside(np.concatenate([head, tail]), sig[-1][LONG, :len(x)], KE, f"{name}: cut at {cut}")
        err = np.abs(state.cpu().numpy()[0].astype(fm.WIDE) - want).astype(np.float64)
        assert (err <= KE).all(), f"{name}: the state behind the pieces (cut at {cut})"
    # a row without frames leaves its state alone
    state = torch.full((1, nsec, 4), 0.25, dtype=torch.float64, device="cuda")
    assert launch(name, [x[:0]], state=state)[0].size == 0
    assert (state.cpu().numpy() == 0.25).all()


@pytest.mark.parametrize("p", [0, C16 + 1, T + 7])
@pytest.mark.parametrize("name", ["highpass_20", "voice"])
def test_a_nan_spoils_only_what_lies_behind_it(name, p):
    rows, _ = rows_in()
    sig, E = model(name)
    x = rows[LONG]
    bad = x.copy()
    bad[p] = np.nan
    out = launch(name, [x, bad, x])                             # (launch checks the sentinels)
    want, KE = sig[-1][LONG, :len(x)], K * E[LONG]
    inside(out[0], want, KE, f"{name}: the row in front of the NaN's")
    inside(out[2], want, KE, f"{name}: the row behind the NaN's")
    inside(out[1][:p], want[:p], KE, f"{name}: the frames in front of the NaN at {p}")
    assert (out[0].view(np.uint32) == out[2].view(np.uint32)).all()


def test_filter_tensor_and_its_valid_lengths():
    sos = CASCADES["voice"]
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.0, 1.0, (2, 3, 1000)).astype(np.float32)
    valid = np.array([[1000, 0, 17], [999, 1, 512]])
    sig = fm.run(sos, x.reshape(6, 1000))
    KE = K * fm.bound(sos)
    t = torch.from_numpy(x).cuda()
    y = afgpu.filter_tensor(t, sos).cpu().numpy().reshape(6, 1000)
    inside(y.reshape(-1), sig[-1].reshape(-1), KE, "filter_tensor")
    z = afgpu.filter_tensor(t, sos, valid=valid).cpu().numpy().reshape(6, 1000)
    for k, n in enumerate(valid.reshape(-1)):
        assert (z[k, :n].view(np.uint32) == y[k, :n].view(np.uint32)).all() and (z[k, n:].view(np.uint32) == 0).all()
    state = torch.zeros((2, 3, len(sos), 4), dtype=torch.float64, device="cuda")
    a = afgpu.filter_tensor(t[..., :300].contiguous(), sos, state=state)
    b = afgpu.filter_tensor(t[..., 300:].contiguous(), sos, state=state)
    inside(torch.cat([a, b], dim=-1).cpu().numpy().reshape(-1), sig[-1].reshape(-1), KE, "filter_tensor in two pieces")
    u = t.clone()
    assert afgpu.filter_tensor(u, sos, out=u) is u and (u.cpu().numpy().reshape(6, 1000).view(np.uint32) == y.view(np.uint32)).all()
    with pytest.raises(afgpu.AfgError):
        afgpu.filter_tensor(t, [(1.0, 0.0, 0.0, -2.0, 1.0)])
