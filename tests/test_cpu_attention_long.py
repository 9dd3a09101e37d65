"""The case table, rounding model and fp32 restatement of the long-sequence attention tests (tests/attention_long_util.py), checked without
a GPU: the table holds the listed cases, the rounding model stays within a third of every tolerance of tests/attention_util.py, the late
regimes move the running maximum, and the comparison functions accept the right restatement and reject every deliberately wrong one."""
import re

import pytest
import torch

import attention_long_util as lu
import attention_util as au


def test_tolerances_and_references_are_attention_utils_own():
    for name in ("FWD_ABS_V", "FWD_CLOSE", "BWD_ABS_THIRD", "BWD_REL_RMS", "DBIAS_RTOL", "DBIAS_ABS", "EPS16", "SCALE"):
        assert getattr(lu, name) is getattr(au, name), name
    for name in ("fwd_failures", "bwd_failures", "dbias_failures"):
        assert getattr(lu, name) is getattr(au, name), name
    assert (au.FWD_ABS_V, au.FWD_CLOSE, au.BWD_ABS_THIRD, au.BWD_REL_RMS, au.DBIAS_RTOL, au.DBIAS_ABS) == (6.0, (4.0, 6.0), 8.0, 3.0, 1e-3, 8.0)


def test_table_holds_the_listed_cases():
    t = lu.long_table()
    assert lu.UNIT_L == (65, 66, 127, 128, 129, 145, 191, 192, 193, 197, 256, 257, 577) and lu.SHAPE == (2, 2)
    assert lu.MAG_L == (65, 128, 129, 197) and lu.LATE_L == (129, 197) and lu.LATE_FROM == {"late64": 64, "late128": 128}
    assert set(lu.GRID) == {(1, 1), (1, 12), (7, 3), (257, 1)} and lu.GRID_L == (65, 197) and lu.NEIGHBOUR_L == (65, 197)
    assert len(t) == len(set(t)) == 13 + 2 * 4 + 2 * 2 + 4 * 2
    assert all(lu.LONG_MIN_L <= L <= lu.LONG_MAX_L for _, _, L, _ in t) and lu.LONG_MAX_L >= 577


def test_rounding_model_uses_at_most_a_third_of_every_tolerance():
    bad = []
    for regime, n, L, heads in lu.long_table():
        for dt in au.DTYPES:
            c = lu.long_case(regime, n, L, heads, dt)
            m = lu.model_long(c)
            zero = torch.zeros(3 * heads * 64)
            f = (au.fwd_failures(m["out"], c["out"], c["vmax"], dt, frac=1 / 3) + au.bwd_failures(m["dqkv"], c["dqkv"], heads, dt, frac=1 / 3)
                 + au.dbias_failures(m["dbias"].float(), c, zero, frac=1 / 3))
            bad += [f"{regime} n={n} L={L} heads={heads} {dt}: {x}" for x in f]
    assert not bad, "\n".join(bad)


def test_docstring_table_is_what_the_measurement_gives():
    rows = re.findall(r"^    long +(\w+) +(.*?) +(\d\.\d{3})$", lu.__doc__, re.M)
    doc = {(a, b): float(c) for a, b, c in rows}
    got = lu.measure()
    assert set(doc) == set(got)
    for key, v in got.items():
        assert abs(doc[key] - v) <= 6e-4 and v <= 1 / 3, (key, doc[key], v)


def test_regimes_are_what_they_claim():
    for regime, n, L, heads in lu.long_table():
        for dt in au.DTYPES:
            s = au.logits64(lu.long_case(regime, n, L, heads, dt)["qkv"], n, L, heads)
            if regime == "offset":
                assert s.max(-1).values.min().item() > au.EXPF_OVERFLOW
            if regime == "peaked":
                assert (torch.softmax(s, -1).max(-1).values > 0.5).double().mean().item() > 0.5
            if regime in lu.LATE_FROM:
                # the largest logit of (nearly) every row lies in a block behind the first one (two), well above what came before
                k0 = lu.LATE_FROM[regime]
                gap = s[..., k0:].max(-1).values - s[..., :k0].max(-1).values
                assert (gap > 2.0).double().mean().item() > 0.9, (regime, L, dt, gap.min().item())


# ------------------------------------------------------------------------------------------------ mutants
MUTANT_CASES = {
    "key_mask_edge": [("unit", 2, L, 2) for L in (65, 128, 192)],                  # 128, 192: the extra key opens a block of its own
    "no_rescale": [(r, 2, L, 2) for r in lu.LATE_FROM for L in lu.LATE_L],
    "query_tail": [("unit", 2, L, 2) for L in (65, 129, 197)] + [("unit", 7, 65, 3)],
    "img_head_swap": [("unit", 7, 65, 3), ("unit", 1, 197, 12), ("unit", 257, 65, 1)],
    "no_scale_ds": [("unit", 2, 65, 2), ("peaked", 2, 197, 2), ("unit", 2, 577, 2)],
}


def test_unmutated_restatement_is_accepted_everywhere():
    bad = []
    for regime, n, L, heads in lu.long_table():
        for dt in au.DTYPES:
            f = lu.restatement_failures(lu.long_case(regime, n, L, heads, dt))
            bad += [f"{regime} n={n} L={L} heads={heads} {dt}: {x}" for x in f]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mutant", lu.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    """every deliberate error is noticed on at least one case of the committed table, in both dtypes"""
    table = lu.long_table()
    caught = {dt: [] for dt in au.DTYPES}
    for case in MUTANT_CASES[mutant]:
        assert case in table, case
        for dt in au.DTYPES:
            if lu.restatement_failures(lu.long_case(*case, dt), mutant):
                caught[dt].append(case)
    assert all(caught.values()), f"{mutant} passes the comparison functions: caught only at {caught}"


def test_query_tail_mutant_is_what_the_sentinel_rows_look_for():
    """the write past L next to sentinel rows: what tests/test_gpu_attention_long.py's neighbour test finds behind the last image"""
    dt = torch.float16
    c = lu.long_case("unit", 2, 65, 2, dt)
    good = lu.restate32_long(c["qkv"], c["dout"], 2, 65, 2, dt)
    wrong = lu.restate32_long(c["qkv"], c["dout"], 2, 65, 2, dt, "query_tail")
    assert not au.bitwise_failures(good["out"][:65], wrong["out"][:65], "first image")         # its own rows are right ...
    assert au.bitwise_failures(good["out"][65:], wrong["out"][65:], "last image")              # ... and its tail overwrote its neighbour's
