"""Host tests of tests/struct_exact.py, the reference of the structured loop path's GPU tests (tests/test_gpu_struct_injected.py):

* the float64 restatement of the four stages stays inside every derived bound on every case of the table (ratio <= 1);
* each of the mistakes a kernel can make (sx.MUTATIONS), applied to the restatement, breaks a bound on every case of its class;
* the bounds are sharp: 1e-11 of amp lam (H) and of amp y_std^2 per entry (covariance), px.SHARP_MEAN of the mean; the n == Lg
  sets only in absolute terms (sx.SHARP_ABS), and their mean's bound may be vacuous -- theirs alone;
* the length scales put the basis' rank into the class a family names, with margins that make it no matter of rounding, in the
  float64 restatement of the device's pivoted Cholesky and in the extended one;
* the table reaches both values of every launch switch of the path and all six K extents, by the plans of csrc/gpet_iter_plan.h
  (through the shim of tests/test_iter_plan.py).

The ratios are printed (pytest -s)."""
import ctypes as C

import numpy as np
import pytest

from tests import posterior_exact as px
from tests import struct_exact as sx
from tests.test_iter_plan import dims, shim  # noqa: F401  (the fixture)

FAMS = sorted(sx.FAMILIES)


@pytest.mark.parametrize("fam", FAMS)
def test_restatement_inside_the_bounds_and_mutations_outside(fam):
    for c in sx.cases_of(fam):
        out, sharp = sx.check_all(c, sx.restate(c))
        print("%-16s %s" % (c, "  ".join("%s %.3g" % kv for kv in out.items())))
        print("%-16s sharpness: %s" % ("", "  ".join("%s %.3g" % kv for kv in sharp.items())))
        assert px.within(out), (c, {k: v for k, v in out.items() if not v <= 1})
        if sx.is_full(c):
            assert sharp["H"] <= sx.SHARP_ABS and sharp["cov"] <= sx.SHARP_ABS, (c, sharp)
        else:
            assert sharp["H"] <= 1e-11 and sharp["cov"] <= 1e-11 and sharp["mean"] <= px.SHARP_MEAN, (c, sharp)
        assert sharp["trunc"] <= 0.1, (c, sharp)  # (the truncation term is a small part of the end-to-end bound)
        for mut in sx.MUTATIONS:
            if not sx.applies(mut, c):
                continue
            bad, _ = sx.check_all(c, sx.restate(c, mut))
            k, v = sx.worst({k: v for k, v in bad.items() if not (sx.is_full(c) and k in ("mean", "e2e_mean"))})
            print("%-16s %-10s caught by %s: %.3g" % ("", mut, k, v))
            assert not v <= 1.0, (c, mut, bad)


def test_only_the_full_grid_sets_have_a_vacuous_mean_bound():
    full = [c for c in sx.ALL_CASES if sx.is_full(c)]
    assert {c.fam for c in full} == {"full64", "full130"}
    for c in full:
        _, sharp = sx.check_all(c, sx.restate(c))
        print(c, sharp)


@pytest.mark.parametrize("fam", FAMS)
def test_length_scales_put_the_rank_into_its_class(fam):
    c = sx.cases_of(fam)[0]
    r, last, rem = sx.basis_margins(c)
    rx, lastx, remx = sx.ext_pchol(c.Lg, c.x_st, c.length)
    print("%s: l = %g  rank %d (extended: %d)  last pivot / tol %.2f (%.2f)  remainder / tol %.3f (%.3f)" % (fam, c.length, r, rx, last, lastx, rem, remx))
    assert c.r0[0] <= r <= c.r0[1] and rx == r
    assert min(last, lastx) >= 1.8 and max(rem, remx) <= 0.6
    assert r < min(c.factor_cap, c.Lg)  # (a rank that reaches the capacity takes the batch off the path)
    assert sx.restated_basis(c.Lg, c.x_st, c.length)[0].shape == (r, c.Lg)


def test_table_reaches_every_launch_class(shim):
    """fit_plan.in_lds (small | blocked form), struct_h_plan.l_in_lds, the idx_in_lds condition of k_struct_H
    (4 n <= 8 r_cap), k_extent(r0) and the column tiles of k_struct_rows (SR_TJ = 64), per case, from the headers."""
    seen = {"in_lds": set(), "l_in_lds": set(), "idx_in_lds": set(), "ks": set(), "r0": set(), "tiles": set(), "blocks": set(), "class": set()}
    for fam in FAMS:
        c0 = sx.cases_of(fam)[0]
        r0 = sx.basis_margins(c0)[0]
        r_cap = min(c0.factor_cap, c0.Lg)
        d = dims(n_cap=c0.n_cap, r0_max=r0, r_cap=r_cap, Lg=c0.Lg)
        o = (C.c_int * 2)()
        shim.shim_fit(d, o)
        in_lds = bool(o[0])
        assert in_lds == (c0.n_cap <= 128)
        seen["in_lds"].add(in_lds)
        if in_lds:
            shim.shim_struct_h(d, o)
            seen["l_in_lds"].add(bool(o[0]))
            for c in sx.cases_of(fam):
                seen["idx_in_lds"].add(4 * c.n <= 8 * r_cap)
        else:
            seen["blocks"].add((c0.n_cap + 63) // 64)
            seen["r0"].add(r0)
        shim.shim_k_extent(r0, o)
        seen["ks"].add(o[0])
        seen["tiles"].add((c0.Lg % 64 == 0, (c0.Lg + 63) // 64))
        seen["class"].update(k for k in sx.R0_CLASSES if k[0] <= r0 <= k[1])
    assert seen["in_lds"] == seen["l_in_lds"] == seen["idx_in_lds"] == {True, False}
    assert seen["ks"] == {8, 12, 16, 18, 20, 24}
    assert {15, 16, 17} <= seen["r0"] and any(49 <= r <= 80 for r in seen["r0"]) and any(r >= 81 for r in seen["r0"])
    assert seen["blocks"] == {3, 4, 5}  # n_cap 129 .. 192, 193 .. 256, 257
    assert {(False, 1), (True, 1), (False, 2), (False, 3)} <= seen["tiles"]  # Lg = 63, 64, 65, 130
    assert seen["class"] == set(sx.R0_CLASSES)
    # the counts of the two forms, under every capacity (counts above a capacity left out)
    ns = {(c.n_cap, c.n) for c in sx.ALL_CASES}
    small = lambda cap: {2, 3, 63, 64, 65, cap - 1, cap}
    blocked = lambda cap: {n for n in (2, 63, 64, 65, 128, 129, 191, 192, 193, cap - 1, cap) if n <= cap}
    for cap in (100, 128):
        assert {(cap, n) for n in small(cap)} <= ns, cap
    for fam, cap in (("b129", 129), ("b192", 192), ("b193", 193), ("b257", 257), ("b257r", 257)):
        assert {c.n for c in sx.cases_of(fam)} == blocked(cap), fam
    assert any(c.dup for c in sx.cases_of("s100")) and any(c.dup for c in sx.cases_of("b129"))
