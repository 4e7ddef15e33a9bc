"""afg_slide_cmn_hip against tests/slidecmn_model.py, bit for bit.  Both planes start out as the word 0x7fc0dead -- a NaN for
whoever reads a float outside its slab, a sentinel for whoever stores one -- with guard words round every slab and, where the
pitch is larger than the slab needs, behind every row; the whole output plane is compared as bit patterns, so a store outside
a slab, a frame behind n_frames that was touched and a read of a guard all show.  Every launch runs behind the LDS fill probe
(conftest.py and Launch.run).  A tile is 32 frames: 33, 65, 97 and 129 frames lie past tile edges.

An infinite frame: with norm_vars var is inf - inf, so exactly the outputs whose window holds the frame are NaN; without it the
definition makes mean infinite and finite elements of such a window the opposite infinity, not NaN (include/afg.h) -- there
the test holds the device to the model's bits and to NaN in the infinite frame itself."""
import numpy as np
import pytest
import torch

import afgpu
import slidecmn_model as model

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x7fc0dead)
GUARD = 5
FRAMES = [1, 2, 31, 32, 33, 63, 64, 65, 97, 129]
WINDOWS = [1, 2, 31, 32, 33, 64, 300, 600]
MODES = [(True, 100), (False, 1), (False, 100)]                  # (center, min_cmn_window): the minimum plays no part when centred
LAYOUTS = {"frames-major": afgpu.CMN_FRAMES_MAJOR, "col-major": afgpu.CMN_COL_MAJOR}


class Launch:
    """slabs of one parameter set, laid one behind the other in a plane of sentinel words"""

    def __init__(self, cols, layout, cmn_window, min_cmn_window, center, norm_vars):
        self.cols, self.col_major = cols, layout == afgpu.CMN_COL_MAJOR
        self.kw = dict(cmn_window=cmn_window, min_cmn_window=min_cmn_window, center=center, norm_vars=norm_vars)
        self.prm = afgpu.cmn_params(cols, layout=layout, **self.kw)
        self.slabs, self.at = [], 0

    def add(self, x, extra_pitch=0, rows_held=None):
        """x [N, cols]; rows_held: the frames the plane has room for (>= N: frames behind n_frames that must stay)"""
        x = np.ascontiguousarray(x, np.float32).reshape(-1, self.cols)
        held = x.shape[0] if rows_held is None else rows_held
        pitch = (held if self.col_major else self.cols) + extra_pitch
        self.at += GUARD
        self.slabs.append((self.at, pitch, x))
        self.at += pitch * (self.cols if self.col_major else held)
        return len(self.slabs) - 1

    def index(self, k):
        """the plane indices of slab k's elements, [N, cols]"""
        off, pitch, x = self.slabs[k]
        t, c = np.meshgrid(np.arange(x.shape[0]), np.arange(self.cols), indexing="ij")
        return off + (c * pitch + t if self.col_major else t * pitch + c)

    def plane(self, values):
        """a sentinel plane with values[k] [N, cols] in slab k's elements"""
        p = np.full(self.at + GUARD, SENTINEL, np.uint32)
        for k, v in enumerate(values):
            if v.size:
                p[self.index(k)] = np.ascontiguousarray(v, np.float32).view(np.uint32)
        return p

    def records(self, out_shift=0):
        rec = np.zeros(len(self.slabs), afgpu.CMN_SLAB_DTYPE)
        for k, (off, pitch, x) in enumerate(self.slabs):
            rec[k]["in_off"], rec[k]["out_off"], rec[k]["pitch"], rec[k]["n_frames"] = off, off + out_shift, pitch, x.shape[0]
        return rec

    def want(self):
        return [model.sliding_cmn(x, **self.kw) for _, _, x in self.slabs]

    def run(self, in_place, out_shift=0):
        """the output plane's words behind one launch"""
        rec = self.records(0 if in_place else out_shift)
        tiles = afgpu.cmn_layout(rec)
        src = self.plane([x for _, _, x in self.slabs])
        d_in = torch.from_numpy(src.view(np.int32)).cuda()
        d_out = d_in if in_place else torch.from_numpy(np.full(src.size + out_shift, SENTINEL, np.uint32).view(np.int32)).cuda()
        nbytes = afgpu.cmn_work_bytes(tiles, self.cols)
        work = torch.full((max(nbytes, 8) // 8,), float("nan"), dtype=torch.float64, device="cuda")
        d_rec = torch.from_numpy(rec.view(np.uint8)).cuda()
        afgpu.lds_fill()
        afgpu.slide_cmn(len(rec), d_rec, tiles, self.prm, d_in, d_in.numel(), d_out, d_out.numel(), work, nbytes)
        torch.cuda.synchronize()
        if not in_place:                                         # the input is only read
            assert (d_in.cpu().numpy().view(np.uint32) == src).all()
        return d_out.cpu().numpy().view(np.uint32)

    def check(self, want=None, out_shift=3):
        """out of place and in place: the whole plane, word for word.  Returns the results per slab."""
        want = self.want() if want is None else want
        exp = self.plane(want)
        got = self.run(False, out_shift)
        assert (got[:out_shift] == SENTINEL).all()
        bad = np.flatnonzero(got[out_shift:] != exp)
        assert bad.size == 0, ("out of place", len(bad), bad[:5].tolist())
        got = self.run(True)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, ("in place", len(bad), bad[:5].tolist())
        return want


def noise(rng, n, cols):
    return (rng.standard_normal((n, cols)) * 3.0 + 1.0).astype(np.float32)


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("cols", [1, 23, 80, 81, 257])
def test_every_shape_and_option_gives_the_models_bits(gpu, cols, name):
    rng = np.random.default_rng(cols * 7 + len(name))
    data = [noise(rng, n, cols) for n in FRAMES]
    for w in WINDOWS:
        for center, m in MODES:
            for norm_vars in (False, True):
                run = Launch(cols, LAYOUTS[name], w, m, center, norm_vars)
                for k, x in enumerate(data):
                    run.add(x, extra_pitch=(0, 3)[k & 1], rows_held=x.shape[0] + (0, 0, 2)[k % 3])
                    if k == 4:
                        run.add(np.zeros((0, cols), np.float32), rows_held=3)     # a slab without frames between the others
                run.check()


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_a_slab_gives_the_same_bits_wherever_it_stands(gpu, name):
    rng = np.random.default_rng(11)
    twin, a, b = noise(rng, 97, 81), noise(rng, 40, 81), noise(rng, 65, 81)
    b[3] = np.nan
    kw = dict(cmn_window=33, min_cmn_window=100, center=True, norm_vars=True)
    first = Launch(81, LAYOUTS[name], **kw)
    ks = [first.add(twin), first.add(a), first.add(twin, extra_pitch=7)]
    res = first.check()
    assert (res[ks[0]].view(np.uint32) == res[ks[2]].view(np.uint32)).all()
    second = Launch(81, LAYOUTS[name], **kw)
    second.add(b)
    second.add(np.zeros((0, 81), np.float32))
    k = second.add(twin, extra_pitch=1)
    got = second.run(False)
    assert (got[second.index(k)] == res[ks[0]].view(np.uint32)).all()


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("center,cmn_window,min_cmn_window", [(True, 300, 100), (False, 600, 100), (True, 31, 1)])
def test_special_values(gpu, name, center, cmn_window, min_cmn_window):
    """column 0 constant (the floor with norm_vars), 1 one NaN, 2 one +inf, 3 signed zeros, 4 noise"""
    n, at = 700, 350
    rng = np.random.default_rng(5)
    x = noise(rng, n, 5)
    x[:, 0] = np.float32(0.3)
    x[at, 1] = np.nan
    x[at, 2] = np.inf
    x[:, 3] = np.where(rng.integers(0, 2, n) == 1, np.float32(-0.0), np.float32(0.0))
    holds = np.array([ws <= at < we for ws, we in (model.window(t, n, cmn_window, min_cmn_window, center) for t in range(n))])
    assert 0 < holds.sum() < n
    for norm_vars in (False, True):
        run = Launch(5, LAYOUTS[name], cmn_window, min_cmn_window, center, norm_vars)
        run.add(x)
        y = run.check()[0]                                       # the device's bits are these
        nan = np.isnan(y)
        assert (nan[:, 1] == holds).all() and not nan[:, [0, 3, 4]].any()
        assert (y.view(np.uint32)[nan] == 0x7fc00000).all()
        if norm_vars:
            assert (nan[:, 2] == holds).all()
            assert np.abs(y[:, 0]).max() <= 1e-2                 # the floor: (x - mean) * 1e5 of a rounding residue, not a division by 0
        else:
            others = np.flatnonzero(holds & (np.arange(n) != at))
            assert nan[at, 2] and nan[:, 2].sum() == 1 and (y[others, 2] == -np.inf).all()


def refusal_cases():
    def base():
        run = Launch(4, afgpu.CMN_FRAMES_MAJOR, 5, 1, True, True)
        rng = np.random.default_rng(2)
        run.add(noise(rng, 40, 4))
        run.add(noise(rng, 33, 4), extra_pitch=2)
        return run

    def edit(field, k, value):
        def f(run, rec, args):
            rec[k][field] = value
        return f

    def prm(field, value):
        def f(run, rec, args):
            setattr(run.prm, field, value)
        return f

    def arg(name, value):
        def f(run, rec, args):
            args[name] = value(args) if callable(value) else value
        return f

    return base, {
        "a slab past the input": arg("in_floats", lambda a: a["in_floats"] - GUARD - 3),   # (the last row has 2 floats of pitch behind it)
        "a slab past the output": arg("out_floats", lambda a: a["out_floats"] - GUARD - 3),
        "an offset past the plane": edit("in_off", 1, 1 << 40),
        "a pitch below the columns": edit("pitch", 0, 3),
        "cmn_window 0": prm("cmn_window", 0),
        "cmn_window above the limit": prm("cmn_window", (1 << 20) + 1),
        "min_cmn_window 0": prm("min_cmn_window", 0),
        "center 2": prm("center", 2),
        "norm_vars 2": prm("norm_vars", 2),
        "cols 0": prm("cols", 0),
        "cols above the limit": prm("cols", 1025),
        "an unknown layout": prm("layout", 2),
        "two outputs that overlap": edit("out_off", 1, GUARD + 8),
        "an output over another slab's input in the same plane": "same-plane",
        "a first_tile the layout did not give": edit("first_tile", 1, 1),
        "a tile count the layout did not give": arg("tiles", lambda a: a["tiles"] + 1),
        "a workspace too small": arg("work_bytes", lambda a: a["work_bytes"] - 16),
        "a reserved word set": edit("reserved", 0, (0, 1, 0)),
    }


BASE, REFUSALS = refusal_cases()


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_write_nothing(gpu, what):
    run = BASE()
    rec = run.records()
    tiles = afgpu.cmn_layout(rec)
    src = run.plane([x for _, _, x in run.slabs])
    args = dict(in_floats=src.size, out_floats=src.size, tiles=tiles, work_bytes=afgpu.cmn_work_bytes(tiles, 4))
    same_plane = REFUSALS[what] == "same-plane"
    if same_plane:
        rec[1]["out_off"] = rec[0]["in_off"] + 4                 # slab 1 would write over what slab 0 reads
    else:
        REFUSALS[what](run, rec, args)
    d_in = torch.from_numpy(src.view(np.int32)).cuda()
    d_out = d_in if same_plane else torch.from_numpy(np.full(src.size, SENTINEL, np.uint32).view(np.int32)).cuda()
    work = torch.zeros(args["work_bytes"] // 8 + 2, dtype=torch.float64, device="cuda")
    if what != "a workspace too small":                          # (the workspace is the entry's own argument)
        with pytest.raises(afgpu.AfgError) as e:
            afgpu.cmn_check_slabs(rec, args["tiles"], run.prm, args["in_floats"], args["out_floats"], same_plane)
        assert "invalid argument" in str(e.value)
    with pytest.raises(afgpu.AfgError) as e:
        afgpu.slide_cmn(len(rec), torch.from_numpy(rec.view(np.uint8)).cuda(), args["tiles"], run.prm, d_in, args["in_floats"], d_out,
                        args["out_floats"], work, args["work_bytes"])
    assert "invalid argument" in str(e.value)
    torch.cuda.synchronize()
    assert (d_in.cpu().numpy().view(np.uint32) == src).all()
    if not same_plane:
        assert (d_out.cpu().numpy().view(np.uint32) == SENTINEL).all()
    assert (work.cpu().numpy() == 0).all()


def test_the_tensor_call(gpu):
    rng = np.random.default_rng(3)
    x = noise(rng, 2 * 3 * 70, 9).reshape(2, 3, 70, 9)
    valid = np.array([70, 0, 33, 1, 64, 69])
    kw = dict(cmn_window=20, min_cmn_window=5, center=False, norm_vars=True)
    want = np.zeros_like(x)
    for k, v in enumerate(valid):
        want.reshape(6, 70, 9)[k, :v] = model.sliding_cmn(x.reshape(6, 70, 9)[k, :v], **kw)
    t = torch.from_numpy(x).cuda()
    y = afgpu.sliding_cmn_tensor(t, valid_frames=valid, **kw)
    assert (y.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all() and (t.cpu().numpy() == x).all()
    # layout "cols": the transposed tensor gives the transposed result; in place through out=
    tc = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 1, 3, 2))).cuda()
    full = afgpu.sliding_cmn_tensor(tc, layout="cols", out=tc, **kw)
    assert full is tc
    whole = np.stack([model.sliding_cmn(s, **kw) for s in x.reshape(6, 70, 9)]).reshape(x.shape)
    assert (tc.cpu().numpy().view(np.uint32) == np.ascontiguousarray(whole.transpose(0, 1, 3, 2)).view(np.uint32)).all()
    with pytest.raises(afgpu.AfgError):
        afgpu.sliding_cmn_tensor(t, cmn_window=0)
    assert tuple(afgpu.sliding_cmn_tensor(torch.zeros(0, 5, 4, device="cuda")).shape) == (0, 5, 4)
