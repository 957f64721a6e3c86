"""The sample GEMM (csrc/gpet_k_sample_score.inc: k_sample_gemm_mfma_r / _rl and k_sample_gemm_mfma) bit for bit on injected
inputs: samples = (Z[:, :rank] @ factor + mean) * y_s.

The inputs make every product and every partial sum EXACT in float64 -- the normals are integers in [-8, 8], factor and mean
entries integer multiples of 2^-20 in [-4, 4], y_s = 1.5: a sum of up to 100 products is a multiple of 2^-20 below 2^12, 32
bits -- so the order of accumulation cannot matter and any difference from numpy is a wrong ELEMENT: a column dealt to the wrong
accumulator, a mean of the neighbouring column, a stale factor row, a normal beyond the rank.  With float32 samples the expected
matrix is numpy's rounding of the same exact one; the 2^-20 grain makes that rounding real.

Per batch: gpet_gp_fit_predict once (the stage needs a fit), then mean and y_s overwritten, and for every rank, largest first:
a full-capacity factor of NaN, the rank-row factor over it, normals with NaN in every column from the rank on, a sample matrix
of NaN, gpet_gp_sample.  Whatever the kernel must not read, or fails to write, is NaN in the output.

Which kernel a case reaches follows from the batch's capacities (launch_sample in gpet_k_launch.inc): capacities of at most 96
take the register form with KS = ceil(capacity / 4) rounded up to one of 8, 12, 16, 18, 20 (_rl), 24 (_rl); a factor row
capacity above 96 the generic form.  Every case asserts the capacities gpet_batch_info reports, so that a change of the sizing
rules cannot move a case to another kernel unnoticed.

The batches come from tests/injected_batch.py (the constructor's own parameter functions and _lib.Batch) rather than from
GP_Edge_Tracing: the constructor, like the reference's, turns N_samples <= 100 into 1000, and the case of 63 sample rows (one
row block that is not full, fewer rows than a block of the generic form) needs N_samples = 63.

The register form's trip over more than one 64-column tile per workgroup (the next chunk restaged under the two barriers) runs
in ks8_column_runs alone, KS 8 in f64: everywhere else the launcher gives a workgroup one tile.

Not pinned: the MU_LDS = false instantiations (the posterior mean read from global memory in the epilogue).  They need an edge
wider than 11 456 columns, whose covariance alone is a gigabyte."""
import numpy as np
import pytest

from tests.injected_batch import make_batch

pytestmark = pytest.mark.gpu

M = 8
Y_S = 1.5

# id: (spans [(x_st, Lg)], S, factor_cap, z_cols, (factor_cap, factor_rows_cap) of gpet_batch_info, kernel, ranks per edge)
CASES = {
    "ks8": ([(0, 64)], 129, 32, 0, (32, 32), "r8", [[1, 3, 4, 5, 31, 32]]),
    "ks12_odd_width": ([(0, 65)], 200, 48, 0, (48, 48), "r12", [[33, 47, 48]]),
    "ks16_63_rows": ([(0, 96)], 63, 64, 0, (64, 64), "r16", [[49, 64]]),
    "ks18": ([(0, 130)], 128, 72, 0, (72, 72), "r18", [[65, 70, 72]]),
    "ks20_rl": ([(0, 200)], 257, 80, 0, (80, 80), "rl20", [[73, 80]]),
    "ks24_rl_odd_width": ([(0, 191)], 130, 96, 0, (96, 96), "rl24", [[81, 95, 96]]),
    # 10 column tiles in 8 column runs of 2: the runs 5, 6, 7 of either row block have nothing to do and return
    "ks8_column_runs": ([(0, 577)], 129, 32, 0, (32, 32), "r8", [[5, 32]]),
    "full_width_register": ([(0, 64)], 129, 0, 64, (64, 64), "r16", [[64]]),
    "generic": ([(0, 100)], 129, 0, 100, (96, 100), "generic", [[1, 31, 32, 33, 97, 100]]),
    # three edges on one image, another rank on every edge in every round
    "three_edges": ([(0, 64), (10, 65), (0, 130)], 129, 48, 0, (48, 48), "r12", [[33, 48], [47, 1], [5, 40]]),
}
RUNS = [(c, "f64") for c in CASES] + [(c, "f32") for c in ("ks8", "ks20_rl", "generic")]


def kernel_of(factor_cap, rows_cap):
    """launch_sample's choice, restated."""
    if factor_cap > 96 or rows_cap > 96:
        return "generic"
    ks = (max(factor_cap, rows_cap) + 3) // 4
    for lim, name in ((8, "r8"), (12, "r12"), (16, "r16"), (18, "r18"), (20, "rl20")):
        if ks <= lim:
            return name
    return "rl24"


@pytest.fixture(scope="module")
def amd():
    import gaussian_process_edge_trace_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(amd):
    return amd._lib.Context(0)


def grain(rng, shape):
    """Integer multiples of 2^-20 in [-4, 4]."""
    return rng.integers(-4 * 2 ** 20, 4 * 2 ** 20 + 1, size=shape).astype(np.float64) / 2.0 ** 20


@pytest.mark.parametrize("case,dtype", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_sample_gemm_bit_for_bit(amd, ctx, case, dtype):
    L = amd._lib
    spans, S, factor_cap, z_cols, caps, kernel, ranks = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    N = max(x_st + Lg for x_st, Lg in spans)
    grad = rng.random((M, N)).astype(np.float32)
    b = make_batch(amd, ctx, grad, spans, S, factor_cap, z_cols, dtype)
    try:
        infos = [b.info(e) for e in range(b.B)]
        for (x_st, Lg), inf in zip(spans, infos):
            assert (inf["Lg"], inf["S"]) == (Lg, S)
            assert (inf["factor_cap"], inf["factor_rows_cap"]) == caps, inf
        assert kernel_of(max(i["factor_cap"] for i in infos), max(i["factor_rows_cap"] for i in infos)) == kernel
        b.fit_predict(want_cov=False)
        mus = []
        for e, (x_st, Lg) in enumerate(spans):
            mu = grain(rng, Lg)
            b.write(L.BUF_MEAN, mu, e)
            s = b.scalars(e)
            assert s.status == 0
            s.y_s = Y_S
            b.write_scalars(s, e)
            assert b.scalars(e).y_s == Y_S and np.array_equal(b.read(L.BUF_MEAN, e), mu)
            mus.append(mu)
        if case == "ks12_odd_width":
            # the row pitch (80 elements for 65 columns) is the library's own business: what is written dense is read dense
            dense = np.arange(S * 65, dtype=np.float64).reshape(S, 65) - 1000.0
            b.write(L.BUF_SAMPLES, dense)
            assert np.array_equal(b.read(L.BUF_SAMPLES), dense)
        for rnd in range(len(ranks[0])):
            want = []
            for e, (x_st, Lg) in enumerate(spans):
                r = sorted(ranks[e], reverse=True)[rnd] if len(spans) == 1 else ranks[e][rnd]
                zc, cap = infos[e]["z_cols"], infos[e]["factor_rows_cap"]
                assert 1 <= r <= cap <= zc
                A = grain(rng, (r, Lg))
                Z = rng.integers(-8, 9, size=(S, zc)).astype(np.float64)
                want.append((Z[:, :r] @ A + mus[e]) * Y_S)
                Z[:, r:] = np.nan
                b.write(L.BUF_FACTOR, np.full((cap, Lg), np.nan), e, rows=cap)
                b.write(L.BUF_FACTOR, A, e, rows=r)
                b.write(L.BUF_NORMALS, Z, e)
                b.write(L.BUF_SAMPLES, np.full((S, Lg), np.nan), e)
                assert b.scalars(e).rank == r and np.array_equal(b.read(L.BUF_FACTOR, e), A)
                assert np.array_equal(b.read(L.BUF_NORMALS, e)[:, :r], Z[:, :r]) and np.isnan(b.read(L.BUF_SAMPLES, e)).all()
            b.sample()
            for e, (x_st, Lg) in enumerate(spans):
                r = int(b.scalars(e).rank)
                got = b.read(L.BUF_SAMPLES, e)
                exp = want[e].astype(np.float32).astype(np.float64) if dtype == "f32" else want[e]
                if dtype == "f32":  # (the rounding is real, 38 % of the elements at rank 1 and more above: a condition on the inputs)
                    assert np.mean(exp != want[e]) > 0.25
                assert got.shape == (S, Lg) and not np.isnan(got).any(), (case, e, r, np.argwhere(np.isnan(got))[:8].tolist())
                bad = np.argwhere(got != exp)
                assert bad.size == 0, (case, e, r, len(bad), [(int(i), int(j), got[i, j], exp[i, j]) for i, j in bad[:8]])
    finally:
        b.close()
