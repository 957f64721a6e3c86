"""The sample GEMM on the f32 matrix cores (csrc/gpet_k_sample_f32.inc: k_sample_f32_r<KS> and k_sample_f32; Python
sample_dtype="f32mma", C gpet_batch_set_sample_arith) bit for bit on injected inputs.  The mode is DEFINED as

    z = float32(Z[s][k]), a = float32(A[k][j]);  acc = fmaf(z_k, a_k, acc) for k = 0 .. rank-1 ascending from +0, one
    accumulator per (s, j);  Y[s][j] = float32((float64(acc) + mean[j]) * y_s)

(include/gpet_hip.h) and tests/f32_chain.py evaluates exactly that -- the oracle has no such mode.

The scheme is that of tests/test_gpu_sample_gemm_exact.py, with its CASES table as it stands (every K extent of the register form,
multi-tile column runs, odd widths, 63 sample rows, the generic form, three edges of different ranks) and its poison per round: a
NaN factor of full capacity with the rank-row factor over it, normals that are NaN from the rank on, a NaN sample matrix.  The
inputs are NOT exact this time: standard normals, factor entries 0.3 x standard normal, mean 3 x standard normal, all float64
and not representable in float32, so the narrowing is pinned too; y_s = 1.37.

What makes a wrong order of accumulation a failure instead of a coincidence is a condition on the inputs, asserted at every
edge's largest rank of a case (at least 32 everywhere; at rank 5 a chain in another order still agrees in ~85 % of the elements):
the expected matrix differs in more than 25 % of its elements from each of the chain in descending k, even and odd k in two
accumulators added at the end, an unfused multiply-then-add in float32, and the float64 product rounded once (the "f32" mode's
value), all through the same epilogue.  (Measured on the CPU with these distributions: 0.43-0.78 at ranks 32-100.)

Which kernel a case reaches follows from the batch's capacities (launch_sample_f32 in gpet_k_launch.inc): capacities of at most 96
take the register form with KS = ceil(capacity / 4) rounded up to one of 8, 12, 16, 18, 20, 24, a factor row capacity above 96
the generic form; every case asserts the capacities gpet_batch_info reports."""
import numpy as np
import pytest

from tests.f32_chain import chain
from tests.injected_batch import make_batch
from tests.test_gpu_sample_gemm_exact import CASES, grain

pytestmark = pytest.mark.gpu

M = 8
Y_S = 1.37
# the f32 family's kernel for the f64 family's of the CASES table (one kernel per K extent: no _rl variant)
KERNEL32 = {"r8": "r8", "r12": "r12", "r16": "r16", "r18": "r18", "rl20": "r20", "rl24": "r24", "generic": "generic"}


def kernel_of(factor_cap, rows_cap):
    """launch_sample_f32's choice, restated (none of these edges is too wide for its mean to sit in LDS)."""
    if factor_cap > 96 or rows_cap > 96:
        return "generic"
    ks = (max(factor_cap, rows_cap) + 3) // 4
    for lim in (8, 12, 16, 18, 20):
        if ks <= lim:
            return "r%d" % lim
    return "r24"


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def epilogue(acc, mu, y_s):
    return ((np.asarray(acc).astype(np.float64) + mu) * y_s).astype(np.float32)


def alternatives(Z, A, mu, y_s):
    """What a kernel with another arithmetic would store, through the same epilogue."""
    r = Z.shape[1]
    Zf, Af = Z.astype(np.float32), A.astype(np.float32)
    unfused = np.zeros((Z.shape[0], A.shape[1]), dtype=np.float32)
    for k in range(r):
        unfused = (Zf[:, k, None] * Af[None, k, :]).astype(np.float32) + unfused
    return {
        "descending k": epilogue(chain(Z, A, order=range(r - 1, -1, -1)), mu, y_s),
        "two accumulators": epilogue(chain(Z[:, 0::2], A[0::2]) + chain(Z[:, 1::2], A[1::2]), mu, y_s),
        "unfused": epilogue(unfused, mu, y_s),
        "f64 product rounded once": ((Z @ A + mu) * y_s).astype(np.float32),
    }


def inject(L, b, e, info, Lg, S, A, Z):
    """The round's poison and inputs of edge e: Z [S][z_cols] (made NaN from the rank on), A [r][Lg]."""
    r, cap = A.shape[0], info["factor_rows_cap"]
    Z = Z.copy()
    Z[:, r:] = np.nan
    b.write(L.BUF_FACTOR, np.full((cap, Lg), np.nan), e, rows=cap)
    b.write(L.BUF_FACTOR, A, e, rows=r)
    b.write(L.BUF_NORMALS, Z, e)
    b.write(L.BUF_SAMPLES, np.full((S, Lg), np.nan), e)
    assert b.scalars(e).rank == r and np.array_equal(b.read(L.BUF_FACTOR, e), A)
    assert np.array_equal(b.read(L.BUF_NORMALS, e)[:, :r], Z[:, :r]) and np.isnan(b.read(L.BUF_SAMPLES, e)).all()


def set_mean_and_scale(L, b, e, mu, y_s):
    b.write(L.BUF_MEAN, mu, e)
    s = b.scalars(e)
    assert s.status == 0
    s.y_s = y_s
    b.write_scalars(s, e)
    assert b.scalars(e).y_s == y_s and np.array_equal(b.read(L.BUF_MEAN, e), mu)


def check(got, exp, what):
    exp = np.asarray(exp).astype(np.float64)
    assert got.shape == exp.shape and not np.isnan(got).any(), (what, np.argwhere(np.isnan(got))[:8].tolist())
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, len(bad), [(int(i), int(j), got[i, j], exp[i, j]) for i, j in bad[:8]])


@pytest.mark.parametrize("case", list(CASES))
def test_f32mma_bit_for_bit(amd, ctx, case):
    L = amd._lib
    spans, S, factor_cap, z_cols, caps, kernel, ranks = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)) + 32)
    N = max(x_st + Lg for x_st, Lg in spans)
    grad = rng.random((M, N)).astype(np.float32)
    b = make_batch(amd, ctx, grad, spans, S, factor_cap, z_cols, "f32mma")
    try:
        infos = [b.info(e) for e in range(b.B)]
        for (x_st, Lg), inf in zip(spans, infos):
            assert (inf["Lg"], inf["S"]) == (Lg, S)
            assert (inf["factor_cap"], inf["factor_rows_cap"]) == caps, inf
        assert kernel_of(max(i["factor_cap"] for i in infos), max(i["factor_rows_cap"] for i in infos)) == KERNEL32[kernel]
        b.fit_predict(want_cov=False)
        mus = []
        for e, (x_st, Lg) in enumerate(spans):
            mus.append(3.0 * rng.standard_normal(Lg))
            set_mean_and_scale(L, b, e, mus[e], Y_S)
        for rnd in range(len(ranks[0])):
            want = []
            for e, (x_st, Lg) in enumerate(spans):
                r = sorted(ranks[e], reverse=True)[rnd] if len(spans) == 1 else ranks[e][rnd]
                zc, cap = infos[e]["z_cols"], infos[e]["factor_rows_cap"]
                assert 1 <= r <= cap <= zc
                A = 0.3 * rng.standard_normal((r, Lg))
                Z = rng.standard_normal((S, zc))
                exp = epilogue(chain(Z[:, :r], A), mus[e], Y_S)
                if r == max(ranks[e]):  # the condition on the inputs
                    assert r >= 32
                    for name, alt in alternatives(Z[:, :r], A, mus[e], Y_S).items():
                        assert np.mean(alt != exp) > 0.25, (case, e, r, name, np.mean(alt != exp))
                want.append(exp)
                inject(L, b, e, infos[e], Lg, S, A, Z)
            b.sample()
            for e in range(len(spans)):
                check(b.read(L.BUF_SAMPLES, e), want[e], (case, e, int(b.scalars(e).rank)))
    finally:
        b.close()


def test_switching_modes_and_a_bad_argument(amd, ctx):
    """"f32mma", then set_sample_dtype("f32") (which sets the arithmetic back to f64: the f64 product rounded once), then
    "f32mma" again, on the exact 2^-20 grain of tests/test_gpu_sample_gemm_exact.py (every float64 sum exact, so the "f32"
    value is numpy's); gpet_batch_set_sample_arith(b, 7) is GPET_ERR_BAD_ARG and leaves either mode as it was."""
    L = amd._lib
    (x_st, Lg), S, r, y_s = (0, 64), 129, 32, 1.5
    rng = np.random.default_rng(77)
    grad = rng.random((M, Lg)).astype(np.float32)
    b = make_batch(amd, ctx, grad, [(x_st, Lg)], S, 32, 0, "f32mma")
    try:
        info = b.info(0)
        assert (info["factor_cap"], info["factor_rows_cap"]) == (32, 32)
        b.fit_predict(want_cov=False)
        mu = grain(rng, Lg)
        set_mean_and_scale(L, b, 0, mu, y_s)

        def run():
            A = grain(rng, (r, Lg))
            Z = rng.integers(-8, 9, size=(S, info["z_cols"])).astype(np.float64)
            inject(L, b, 0, info, Lg, S, A, Z)
            b.sample()
            exact = (Z[:, :r] @ A + mu) * y_s
            as_chain, as_f32 = epilogue(chain(Z[:, :r], A), mu, y_s), exact.astype(np.float32)
            assert np.mean(as_chain != as_f32) > 0.25  # (the two modes are told apart; 0.70 on the CPU)
            assert np.mean(as_f32.astype(np.float64) != exact) > 0.25
            return b.read(L.BUF_SAMPLES), as_chain, as_f32, exact

        got, as_chain, _, _ = run()
        check(got, as_chain, "f32mma")
        b.set_sample_dtype("f32")
        got, _, as_f32, _ = run()
        check(got, as_f32, "f32 after f32mma")
        b.set_sample_dtype("f32mma")
        got, as_chain, _, _ = run()
        check(got, as_chain, "f32mma again")
        assert b.lib.gpet_batch_set_sample_arith(b.h, 7) == L.ERR_BAD_ARG
        assert b.lib.gpet_batch_set_sample_arith(b.h, -1) == L.ERR_BAD_ARG
        got, as_chain, _, _ = run()
        check(got, as_chain, "f32mma after a refused call")
        b.set_sample_dtype("f64")
        assert b.lib.gpet_batch_set_sample_arith(b.h, 7) == L.ERR_BAD_ARG
        got, _, _, exact = run()
        check(got, exact, "f64 after a refused call")
        # the arithmetic alone set back: f32 storage stays, with the f64 product
        b.set_sample_dtype("f32mma")
        assert b.lib.gpet_batch_set_sample_arith(b.h, L.SAMPLE_ARITH_F64) == 0
        got, _, as_f32, _ = run()
        check(got, as_f32, "arithmetic back to f64, storage f32")
    finally:
        b.close()


def test_the_value_error_names_the_three_modes(amd, ctx):
    b = make_batch(amd, ctx, np.zeros((M, 64), dtype=np.float32), [(0, 64)], 129)
    try:
        with pytest.raises(ValueError, match="'f64', 'f32' or 'f32mma'"):
            b.set_sample_dtype("f16")
    finally:
        b.close()
