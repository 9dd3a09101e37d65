"""The references, case tables and comparison functions of the attention tests (tests/attention_util.py), checked without a GPU: the
fp64 restatement agrees with torch's own attention, the rounding model stays within a third of every tolerance over the whole table,
the regimes are what they claim, and the comparison functions reject every deliberately wrong restatement and accept the right one."""
import importlib.util
import os
import re

import pytest
import torch
import torch.nn.functional as F

import attention_util as au

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fp64_restatement_agrees_with_torch_sdpa():
    for regime, n, L, heads in (("unit", 2, 1, 2), ("unit", 3, 17, 2), ("peaked", 2, 50, 2), ("offset", 2, 64, 2), ("unit", 3, 50, 12)):
        qkv, _ = au.vit_inputs(regime, n, L, heads, torch.float16)
        q, k, v = au.split_heads(qkv.double(), n, L, heads, 3)
        for causal in (False, True):
            want = au.merge_heads(F.scaled_dot_product_attention(q, k, v, is_causal=causal)[None], n, L, heads)
            got = au.attn_ref64(qkv, n, L, heads, causal=causal)
            assert got.dtype == torch.float64 and (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item()), (regime, n, L, heads, causal)


def test_causal_restatement_agrees_with_the_causal_kernel_tests_reference():
    spec = importlib.util.spec_from_file_location("_clip_text_tests", os.path.join(HERE, "test_gpu_clip_text.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    for regime, n, L, heads in (("peaked", 2, 65, 1), ("late", 2, 128, 8), ("offset", 2, 64, 8)):
        qkv = au.causal_inputs(regime, n, L, heads, torch.bfloat16)
        assert torch.equal(au.attn_ref64(qkv, n, L, heads, causal=True), m._attn_ref(qkv, n, L, heads))


def test_rounding_model_uses_at_most_a_third_of_every_tolerance():
    """the one-third condition of attention_util's docstring, over every case of both tables and both dtypes"""
    bad, count = [], 0
    for regime, n, L, heads in au.vit_table():
        for dt in au.DTYPES:
            c = au.vit_case(regime, n, L, heads, dt)
            m = au.model_vit(c)
            zero = torch.zeros(3 * heads * 64)
            f = (au.fwd_failures(m["out"], c["out"], c["vmax"], dt, frac=1 / 3) + au.bwd_failures(m["dqkv"], c["dqkv"], heads, dt, frac=1 / 3)
                 + au.dbias_failures(m["dbias"].float(), c, zero, frac=1 / 3))
            bad += [f"{regime} n={n} L={L} heads={heads} {dt}: {x}" for x in f]
            count += 1
    for regime, n, L, heads in au.causal_table():
        for dt in au.DTYPES:
            c = au.causal_case(regime, n, L, heads, dt)
            f = au.fwd_failures(au.model_causal(c)["out"], c["out"], c["vmax"], dt, frac=1 / 3, close=False)
            bad += [f"causal {regime} n={n} L={L} heads={heads} {dt}: {x}" for x in f]
            count += 1
    assert not bad, "\n".join(bad)
    assert count == 2 * (len(au.vit_table()) + len(au.causal_table())) and len(au.vit_table()) == 64 + 22 + 10 + 6 - 2          # two cases sit in two tables


def test_docstring_table_is_what_the_measurement_gives():
    rows = re.findall(r"^    (vit|causal) +(\w+) +(.*?) +(\d\.\d{3})$", au.__doc__, re.M)
    doc = {(a, b, c): float(d) for a, b, c, d in rows}
    got = au.measure()
    assert set(doc) == set(got)
    for key, v in got.items():
        assert abs(doc[key] - v) <= 6e-4 and v <= 1 / 3, (key, doc[key], v)


def test_tables_hold_the_listed_cases():
    assert au.EVERY_L == tuple(range(1, 65)) and au.EVERY_SHAPE == (2, 2)
    assert au.MAG_L == (1, 15, 16, 17, 32, 33, 48, 49, 50, 63, 64)
    assert set(au.GRID) == {(1, 1), (1, 12), (7, 3), (257, 1), (3, 12)} and au.GRID_L == (17, 50)
    assert au.DBIAS_N == (1, 2, 257) and au.NEIGHBOUR_L == (1, 17, 64) and au.NEIGHBOUR_CAUSAL_L == (1, 65, 128)
    assert au.CAUSAL_L == (64, 65, 128) and au.CAUSAL_HEADS == (1, 8) and au.PAD_ROWS >= 5
    assert set(au.REGIMES) == {"unit", "peaked", "offset"}


def test_inputs_are_16_bit_values_and_pure_functions_of_their_name():
    for dt in au.DTYPES:
        a, da = au.vit_inputs("offset", 2, 17, 2, dt)
        b, db = au.vit_inputs("offset", 2, 17, 2, dt)
        assert a.dtype == dt and da.dtype == dt and torch.equal(a, b) and torch.equal(da, db)
        assert not torch.equal(a, au.vit_inputs("offset", 2, 16, 2, dt)[0][: 2 * 17])


def test_offset_regime_overflows_an_unsubtracted_expf():
    for regime, n, L, heads in au.vit_table() + au.causal_table():
        if regime != "offset":
            continue
        for dt in au.DTYPES:
            qkv = au.vit_case(regime, n, L, heads, dt)["qkv"] if (regime, n, L, heads) in au.vit_table() else au.causal_case(regime, n, L, heads, dt)["qkv"]
            s = au.logits64(qkv, n, L, heads, causal=(regime, n, L, heads) in au.causal_table())
            assert s.max(-1).values.min().item() > au.EXPF_OVERFLOW, (n, L, heads, dt)
            assert torch.isinf(torch.exp(s.max().float()))


def test_peaked_regime_is_peaked():
    for table, causal in ((au.vit_table(), False), (au.causal_table(), True)):
        for regime, n, L, heads in table:
            if regime != "peaked":
                continue
            for dt in au.DTYPES:
                qkv = (au.causal_case if causal else au.vit_case)(regime, n, L, heads, dt)["qkv"]
                p = torch.softmax(au.logits64(qkv, n, L, heads, causal), dim=-1)
                assert (p.max(-1).values > 0.5).double().mean().item() > 0.5, (n, L, heads, dt, causal)


def test_late_maximum_lies_in_the_second_key_block():
    for regime, n, L, heads in au.causal_table():
        if regime != "late":
            continue
        for dt in au.DTYPES:
            s = au.logits64(au.causal_case(regime, n, L, heads, dt)["qkv"], n, L, heads, causal=True)
            assert L == 128 and (s[:, :, 64:].argmax(-1) >= 64).all()
            # "by far": the first block's largest logit is at least 8 below it, so the first block's accumulator shrinks by e^-8
            gap = s[:, :, 64:, 64:].max(-1).values - s[:, :, 64:, :64].max(-1).values
            assert gap.min().item() > 8.0, gap.min().item()


# ------------------------------------------------------------------------------------------------ mutants
# where each deliberate error must be noticed: by the tolerance checks on cases of the committed tables
MUTANT_CASES = {
    "key_mask": [("unit", 2, L, 2) for L in (1, 2, 16, 17)],                          # one extra key among few
    "no_max": [("offset", 2, L, 2) for L in au.MAG_L],                                # overflows everywhere
    "no_scale_ds": [("unit", 2, L, 2) for L in (2, 17, 64)] + [("peaked", 2, 50, 2)],
    "img_head_swap": [("unit", n, 17, h) for n, h in au.GRID if n != h and (n, h) != (257, 1)] + [("unit", 257, 17, 1)],
    "dbias_k_from_v": [("unit", n, L, au.DBIAS_HEADS) for n in au.DBIAS_N for L in au.DBIAS_L],
}


def test_unmutated_restatement_is_accepted_everywhere():
    bad = []
    for regime, n, L, heads in au.vit_table():
        for dt in au.DTYPES:
            f = au.restatement_failures(au.vit_case(regime, n, L, heads, dt))
            bad += [f"{regime} n={n} L={L} heads={heads} {dt}: {x}" for x in f]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mutant", au.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    table = au.vit_table()
    missed = []
    for case in MUTANT_CASES[mutant]:
        assert case in table, case
        for dt in au.DTYPES:
            if not au.restatement_failures(au.vit_case(*case, dt), mutant):
                missed.append((case, dt))
    assert not missed, f"{mutant} passes the comparison functions at {missed}"


def test_mutants_are_rejected_by_the_check_that_is_meant_for_them():
    dt = torch.float16
    c = au.vit_case("unit", 2, 50, 2, dt)
    start = au.dbias_start(2)
    r = au.restate32(c["qkv"], c["dout"], 2, 50, 2, dt, "dbias_k_from_v", start)
    assert not au.fwd_failures(r["out"], c["out"], c["vmax"], dt) and not au.bwd_failures(r["dqkv"], c["dqkv"], 2, dt)
    f = au.dbias_failures(r["dbias"], c, start)
    assert any("K third changed" in x for x in f) and any("column sums of dqkv" in x for x in f)
    r = au.restate32(c["qkv"], c["dout"], 2, 50, 2, dt, "no_scale_ds", start)
    f = au.bwd_failures(r["dqkv"], c["dqkv"], 2, dt)
    assert any(x.startswith("dQ") for x in f) and any(x.startswith("dK") for x in f) and not any(x.startswith("dV") for x in f)
    # the off-by-one key mask next to a NaN image: what the GPU neighbour test looks for (finite, and bitwise equal to an n = 1 run)
    qkv, dout = c["qkv"].clone(), c["dout"].clone()
    qkv[50:], dout[50:] = float("nan"), float("nan")
    alone = au.restate32(c["qkv"][:50], c["dout"][:50], 1, 50, 2, dt)
    good = au.restate32(qkv, dout, 2, 50, 2, dt)
    wrong = au.restate32(qkv, dout, 2, 50, 2, dt, "key_mask")
    for k in ("out", "dqkv"):
        assert not au.finite_failures(good[k][:50], k) and not au.bitwise_failures(good[k][:50], alone[k], k)
        assert au.finite_failures(wrong[k][:50], k) and au.bitwise_failures(wrong[k][:50], alone[k], k)
