"""FastTracker II XM on the host (no device): afg_xm_parse's records against tests/libxm_model.py.  The model steps every
frame and keeps no segments, so the records are compared through what they mean: render_records() below mixes them on the
CPU exactly as the device mixer is specified (include/afg.h) -- stepping positions sequentially, with none of the product's
jumps -- and its output must equal the model's bit for bit; the ticks are compared record for record."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import afgpu
import libxm_model as xm
import xm_bitstream as xb

F = np.float32
SEEDS = list(range(12))


def songs():
    return [xb.random_song(np.random.default_rng(100 + s)) for s in SEEDS]


def render_records(p):
    """The mixer's definition on the CPU: per tick, per segment in order, per frame."""
    out = np.full((p["frames"], 2), np.nan, np.float32)
    data, aux, segs = p["data"], p["aux"], p["segments"]
    for t in p["ticks"]:
        acc = np.zeros((int(t["frames"]), 2), np.float32)
        for g in segs[int(t["seg"]):int(t["seg"]) + int(t["n_seg"])]:
            fl = int(g["flags"])
            w = 2 if fl & afgpu.XM_SEG_16BIT else 1
            smp = data[int(g["sample_off"]):int(g["sample_off"]) + (int(g["last"]) + 1) * w].view(np.int16 if w == 2 else np.int8)
            pos, step = F(g["position"]), F(g["step"])
            for k in range(int(g["frames"])):
                f = int(g["frame"]) + k
                if fl & afgpu.XM_SEG_TABLE and (k == 0 or f % 16 == 0):
                    want = aux[int(g["aux_pos"]) + (f >> 4) - (int(g["frame"]) >> 4)]
                    assert want.view(np.uint32) == np.float32(pos).view(np.uint32)
                a = 0 if not pos >= 0 else min(int(min(pos, F(4e9))), int(g["last"]))
                v = F(F(smp[a]) * F(1 / 32768 if w == 2 else 1 / 128))
                if fl & afgpu.XM_SEG_FADE:
                    u = aux[int(g["aux_fade"]) + k]
                    v = F(u + F(F(F(int(g["fade_count"]) + k) / F(32)) * F(v - u)))
                vl, vr = (aux[int(g["aux_vol"]) + 2 * k], aux[int(g["aux_vol"]) + 2 * k + 1]) if fl & afgpu.XM_SEG_RAMP else (g["vol_l"], g["vol_r"])
                i = f - int(t["frame"])
                acc[i, 0] = F(acc[i, 0] + F(v * vl))
                acc[i, 1] = F(acc[i, 1] + F(v * vr))
                pos = F(pos - step) if fl & afgpu.XM_SEG_BACK else F(pos + step)
        out[int(t["frame"]):int(t["frame"]) + int(t["frames"])] = acc * F(t["scale"])
    return out


@pytest.fixture(scope="module")
def parsed():
    return [(d, afgpu.xm_parse(d)) for d in songs()]


def test_records_render_to_the_models_frames(parsed):
    kinds = {"back": 0, "16bit": 0, "ramp": 0, "fade": 0, "steady": 0, "8bit": 0}
    for data, p in parsed:
        want = xm.decode_batch(data)
        assert not p["capped"] and p["frames"] == len(want) > 0         # the song ends through the model
        got = render_records(p)
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
        fl = p["segments"]["flags"]
        kinds["back"] += int((fl & afgpu.XM_SEG_BACK != 0).sum())
        kinds["16bit"] += int((fl & afgpu.XM_SEG_16BIT != 0).sum())
        kinds["8bit"] += int((fl & afgpu.XM_SEG_16BIT == 0).sum())
        kinds["ramp"] += int((fl & afgpu.XM_SEG_RAMP != 0).sum())
        kinds["fade"] += int((fl & afgpu.XM_SEG_FADE != 0).sum())
        kinds["steady"] += int((fl & (afgpu.XM_SEG_RAMP | afgpu.XM_SEG_FADE) == 0).sum())
    # a generator change must not silently empty a case
    assert all(v > 20 for v in kinds.values()), kinds


def test_ticks_match_the_model(parsed):
    for data, p in parsed:
        pl = xm.Player(xm.load(data))
        pl.generate(p["frames"] + 1, stop_at_loop=True)
        ticks = [t for t in pl.ticks if t[0]]
        if len(ticks) > len(p["ticks"]):
            ticks = ticks[:len(p["ticks"])]                     # (the model noted the tick that raised the loop count)
        assert len(ticks) == len(p["ticks"])
        for w, t in zip(ticks, p["ticks"]):
            assert (w[0], w[2], w[3], w[4]) == (int(t["frames"]), int(t["table_index"]), int(t["row"]), int(t["loop_count"]))
            assert F(w[1]).view(np.uint32) == t["scale"].view(np.uint32)
        segs = p["segments"]
        for t in p["ticks"]:                                    # segments stay inside their tick, channels in order
            s = segs[int(t["seg"]):int(t["seg"]) + int(t["n_seg"])]
            assert (s["frame"] >= t["frame"]).all() and (s["frame"] + s["frames"] <= t["frame"] + t["frames"]).all()
            assert (np.diff(s["channel"].astype(np.int64)) >= 0).all() and (s["frames"] > 0).all()


def test_module_header_fields(parsed):
    for data, p in parsed:
        m = xm.load(data)
        assert (p["channels"], p["length"], p["patterns"], p["instruments"], p["restart"]) == \
               (m.channels, m.length, m.num_patterns, len(m.instruments), m.restart)


def test_probe_and_loader_agree_on_damaged_files():
    rng = np.random.default_rng(7)
    base = songs()[0]
    cases = [base[:n] for n in (0, 17, 59, 60, 61, 80, 336, 400, len(base) // 2, len(base) - 40, len(base) - 1)]
    cases += [rng.integers(0, 256, 4000, dtype=np.uint8).tobytes(), b"Extended Module: " + bytes(200)]
    for _ in range(30):                                         # byte damage in the headers
        b = bytearray(base)
        for _ in range(3):
            b[int(rng.integers(60, min(len(b), 1200)))] = int(rng.integers(0, 256))
        cases.append(bytes(b))
    loaded = 0
    for c in cases:
        m = xm.load(c)
        if m is None:
            with pytest.raises(afgpu.AfgError):
                afgpu.xm_parse(c)
            continue
        loaded += 1
        p = afgpu.xm_parse(c)
        want = xm.decode_batch(c, limit=200000)
        got = render_records(p)[:len(want)]
        assert p["frames"] >= len(want) and (got.view(np.uint32) == want.view(np.uint32)).all()
    assert loaded >= 5                                          # among them the file cut inside its sample data


def test_mod_front_end_still_refuses_xm_headed_files():
    with pytest.raises(afgpu.AfgError):
        afgpu.mod_parse(songs()[0])


def test_single_note_is_hand_checkable():
    """Note 49 (real note 48): period 4608, pow exponent 0, 8363 Hz, step 8363/44100; full volume, centre panning, no
    envelopes.  The first tick is 882 frames; the channel was silent, so the stored cross-fade values are 0 and frame k < 32
    is (k/32 * s_k) * min(g, k/128) * 0.25 with g = sqrt(0.5...) per side."""
    data, smp = xb.single_note()
    p = afgpu.xm_parse(data)
    assert int(p["ticks"][0]["frames"]) == 882 and p["ticks"][0]["scale"] == F(0.25)
    g0 = p["segments"][0]
    assert g0["step"] == F(F(8363) / F(44100)) and g0["position"] == 0
    got = render_records(p)
    pan = F(F(128) / F(255))
    goal = [F(F(1) * xm.sqrtf(F(F(1) - pan))), F(F(1) * xm.sqrtf(pan))]
    pos = F(0)
    checked = 0
    for k in range(128):
        s = F(F(smp[int(pos)]) / F(128))
        if k < 32:
            s = F(F(0) + F(F(F(k) / F(32)) * F(s - F(0))))
        for side in (0, 1):
            gain = min(goal[side], F(k / 128))
            assert got[k, side].view(np.uint32) == F(F(F(0) + F(s * gain)) * F(0.25)).view(np.uint32), (k, side)
        pos = F(pos + g0["step"])
        checked += 1
    assert checked >= 32 and (got[0] == 0).all()
    want = xm.decode_batch(data)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def sample_map(m):
    """sample_off -> sample, laid out as afg_xm_parse's data: instrument order, every sample on an even offset."""
    out, off = {}, 0
    for ins in m.instruments:
        for s in ins.samples:
            off = (off + 1) & ~1
            out[off] = s
            off += s.length * (2 if s.bits == 16 else 1)
    return out


def test_segments_keep_what_the_mixer_relies_on(parsed):
    """The renderer above clamps its index like the device, so a segment that runs over a wrap, a turn or a sample end could
    hide behind the clamp.  Here every segment is stepped without one: forward segments stay below the loop end (or the
    sample end), backward ones above the loop start, ramp segments move on every frame, fade segments end by frame 32."""
    stepped = 0
    for data, p in parsed:
        smp = sample_map(xm.load(data))
        aux = p["aux"]
        for g in p["segments"]:
            s = smp[int(g["sample_off"])]
            fl, n = int(g["flags"]), int(g["frames"])
            assert int(g["last"]) == s.length - 1 and bool(fl & afgpu.XM_SEG_16BIT) == (s.bits == 16)
            assert (s.loop == 2) if fl & afgpu.XM_SEG_BACK else True
            if fl & afgpu.XM_SEG_FADE:
                assert int(g["fade_count"]) + n <= 32
            else:
                assert int(g["fade_count"]) >= 32
            if fl & afgpu.XM_SEG_RAMP:
                v = aux[int(g["aux_vol"]):int(g["aux_vol"]) + 2 * n].reshape(-1, 2)
                assert n <= 128 and (np.abs(np.diff(v.view(np.uint32).astype(np.int64), axis=0)).sum(axis=1) > 0).all()
            pos, step = F(g["position"]), F(g["step"])
            if not (0 <= step <= 1):
                continue                                        # (a step above the loop's length may overshoot: INTEGRATION.md)
            stepped += 1
            limit = s.length if s.loop == 0 else s.loop_end
            start_inside = pos < limit
            for k in range(n):
                assert 0 <= pos < s.length, (k, pos)
                if k and fl & afgpu.XM_SEG_BACK:
                    assert pos > s.loop_start
                if k and not fl & afgpu.XM_SEG_BACK and start_inside:
                    assert pos < limit
                pos = F(pos - step) if fl & afgpu.XM_SEG_BACK else F(pos + step)
    assert stepped > 1000


def test_endless_song_does_not_end_through_the_model():
    """The cap test's song: its first tick is infinitely long (BPM 0), so the loop count stays 0; a bounded prefix of the
    host's records equals the model's frames."""
    data = xb.endless_song()
    pl = xm.Player(xm.load(data))
    got = pl.generate(30000, stop_at_loop=True)
    assert len(got) == 30000 and pl.loop_count == 0 and np.isinf(pl.remaining) and got.any()
