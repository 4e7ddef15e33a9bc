"""tests/cepstra_model.py against itself and against afg_cep_dct, without a GPU: the table against the float64 closed form to
the bit, its orthonormality, the float32 model inside the derived bounds of the float64 statement, the deltas of a ramp, and
five one-place mutants that each leave the bound."""
import math

import numpy as np
import pytest

import afgpu
import cepstra_model as cm


@pytest.mark.parametrize("n_mels", [1, 3, 80, 256])
def test_the_table_is_the_closed_form_rounded_once(n_mels):
    for norm in (cm.DCT_NONE, cm.DCT_ORTHO):
        for lifter in (0.0, 22.0):
            for log_scale in (1.0, math.log(10.0)):
                got = afgpu.cep_dct(n_mels, n_mels, norm, lifter, log_scale)
                want = cm.dct64(n_mels, n_mels, norm, lifter, log_scale).astype(np.float32)
                assert got.shape == (n_mels, n_mels) and got.dtype == np.float32
                assert (got.view(np.uint32) == want.view(np.uint32)).all(), (n_mels, norm, lifter, log_scale)
                few = afgpu.cep_dct(min(2, n_mels), n_mels, norm, lifter, log_scale)          # fewer coefficients: the first rows
                assert (few.view(np.uint32) == want[:len(few)].view(np.uint32)).all()
    assert (afgpu.cep_dct(n_mels, n_mels, "ortho") == afgpu.cep_dct(n_mels, n_mels, afgpu.CEP_DCT_ORTHO)).all()


def test_the_unnormalised_table_is_the_textbook_dct2():
    """2 cos(pi q (2 m + 1) / (2 n)) without the integer reduction: scipy's and torchaudio's type II without norm"""
    n = 80
    q, m = np.arange(n)[:, None], np.arange(n)[None, :]
    assert np.abs(cm.dct64(n, n, cm.DCT_NONE) - 2.0 * np.cos(np.pi * q * (2 * m + 1) / (2.0 * n))).max() < 1e-12
    L = cm.dct64(13, n, cm.DCT_NONE, 22.0)[:, 0] / cm.dct64(13, n, cm.DCT_NONE)[:, 0]                   # the lifter alone
    assert abs(L[0] - 1.0) < 1e-15 and abs(L[11] - 12.0) < 1e-12 and abs(L[1] - (1 + 11 * math.sin(math.pi / 22))) < 1e-12


@pytest.mark.parametrize("n_mels", [1, 3, 80, 256])
def test_the_ortho_table_is_orthonormal(n_mels):
    """D D^T = I up to the rounding of the entries: an entry is off by at most u |d|, so an element of the float32 table's
    product moves by at most sum_m u (|d1||d2| + |d1||d2|) + u^2 ... <= 2 u sum_m |d1[m]||d2[m]| (1 + u) <= 2 u (1 + u) by
    Cauchy-Schwarz on unit rows; the float64 table's own product is within 1e-13 of I"""
    D64 = cm.dct64(n_mels, n_mels, cm.DCT_ORTHO)
    assert np.abs(D64 @ D64.T - np.eye(n_mels)).max() < 1e-13
    D = afgpu.cep_dct(n_mels, n_mels, "ortho").astype(np.float64)
    assert np.abs(D @ D.T - np.eye(n_mels)).max() <= 2 * cm.U * (1 + cm.U) + 1e-13


def slab(rng, n_mels, F):
    """log-mel-like values: log10 of powers between the floor and a loud frame"""
    return rng.uniform(-10.0, 3.0, (n_mels, F)).astype(np.float32)


CASES = [(80, 13, 2, 2, 150), (80, 40, 2, 8, 40), (3, 3, 1, 1, 7), (256, 256, 2, 3, 20), (1, 1, 2, 2, 1), (80, 13, 2, 8, 5)]


@pytest.mark.parametrize("n_mels,n_ceps,order,N,F", CASES)
def test_the_float32_model_lies_inside_the_bound(n_mels, n_ceps, order, N, F):
    rng = np.random.default_rng(n_mels * 1000 + F)
    x = slab(rng, n_mels, F)
    D = afgpu.cep_dct(n_ceps, n_mels, "ortho", 22.0, 1.0)
    got = cm.cepstra32(D, x, order, N)
    want, bound = cm.cepstra64(D, x, order, N)
    assert got.shape == want.shape == ((1 + order) * n_ceps, F)
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    assert (bound[:n_ceps] > 0).all() and bound.max() < 1e-3 * max(np.abs(want).max(), 1.0)       # (a bound that says something)


@pytest.mark.parametrize("mutant", ["clamp", "n0", "gain", "d2c", "swap"])
def test_a_mutant_leaves_the_bound(mutant):
    rng = np.random.default_rng(5)
    x = slab(rng, 80, 150)
    D = afgpu.cep_dct(13, 80, "ortho")
    want, bound = cm.cepstra64(D, x, 2, 2)
    assert (np.abs(cm.cepstra32(D, x, 2, 2).astype(np.float64) - want) <= bound).all()
    off = np.abs(cm.cepstra32(D, x, 2, 2, mutant).astype(np.float64) - want) > bound
    assert off.any()
    if mutant == "clamp":                                        # only the frames whose span reaches over an edge
        t = np.nonzero(off.any(axis=0))[0]
        assert ((t < 4) | (t >= 150 - 4)).all() and off[:13].sum() == 0


@pytest.mark.parametrize("N", range(1, 9))
def test_deltas_of_a_ramp_are_its_slope(N):
    F = 40
    t = np.arange(F, dtype=np.float64)
    slope = np.array([[3.0], [-0.5], [0.0]])
    ramp = (slope * t + np.array([[1.0], [2.0], [7.0]])).astype(np.float32)         # small dyadic numbers: exact in float32
    d1 = cm.delta32(ramp, N).astype(np.float64)
    inner = slice(N, F - N)
    assert (np.abs(d1[:, inner] - slope) <= 2 * cm.U * np.abs(slope)).all()         # g and the product round, nothing else does
    # at the edges the clamped values: sum n (a[min(t + n, F - 1)] - a[max(t - n, 0)]) g in closed form
    want = sum(n * (slope * (np.minimum(t + n, F - 1) - np.maximum(t - n, 0))) for n in range(1, N + 1)) * cm.gain64(N)
    assert (np.abs(d1 - want) <= 2 * cm.U * np.abs(want)).all()
    assert (np.abs(cm.delta64(ramp, N) - want) <= 1e-12).all()
    d2 = cm.delta32(d1.astype(np.float32), N).astype(np.float64)
    assert (np.abs(d2[:, 2 * N:F - 2 * N]) <= 4 * cm.U * np.abs(slope)).all()        # the slope's slope: nothing, up to d1's rounding


def test_layout_counts_tiles():
    rows = np.zeros(6, cm.ROW_DTYPE)
    rows["frames"] = [0, 1, 64, 65, 0, 129]
    assert cm.layout(rows) == 7 and rows["first_tile"].tolist() == [0, 0, 1, 2, 4, 4]
    assert cm.TILE == afgpu.CEP_TILE
