"""The references, input conditions and tolerance table of the BatchNorm / pooling / junction kernel tests (tests/bnpool_util.py),
checked without a GPU: the references agree with torch's own fp64 F.batch_norm / F.max_pool2d autograd, fp32 and fp64 pick the
same window winners and the same signs of z in every case (zero exceptions), the measured constants are what the fp32-CPU
evaluation gives, and the case tables reach the launch paths they claim."""
import numpy as np
import torch
import torch.nn.functional as F

import bnpool_util as bu


def test_references_agree_with_torch_batch_norm_and_max_pool_autograd():
    """every case that reads an fp32 y, through F.batch_norm (its own running-buffer update included) and F.max_pool2d"""
    count = 0
    for what, c in bu.all_act_cases():
        if c["yq"] is not None:
            continue
        n, H, W, C = c["y"].shape
        y = bu._nchw(c["y"], torch.float64).requires_grad_(True)
        g = (torch.ones(C, dtype=torch.float64) if c["gamma"] is None else bu._t(c["gamma"], torch.float64)).requires_grad_(True)
        b = (torch.zeros(C, dtype=torch.float64) if c["beta"] is None else bu._t(c["beta"], torch.float64)).requires_grad_(True)
        rm, rv = bu._t(c["rm"], torch.float64).clone(), bu._t(c["rv"], torch.float64).clone()
        a = F.leaky_relu(F.batch_norm(y, rm, rv, g, b, c["training"], bu.MOMENTUM, c["eps"]), c["slope"])
        k, s, p = (c["pool"][1], c["pool"][1], 0) if c["pool"][0] == "win" else c["pool"][1:]
        out = a if k == 1 else F.max_pool2d(a, k, s, p)
        (out * bu._nchw(c["dout"], torch.float64)).sum().backward()
        pre = c.get("pre") or {}
        for name, got in (("out", bu._nhwc(out)), ("dy", bu._nhwc(y.grad).reshape(-1, C)),
                          ("dgamma", g.grad + (bu._t(pre["dgamma"], torch.float64) if pre else 0)),
                          ("dbeta", b.grad + (bu._t(pre["dbeta"], torch.float64) if pre else 0))):
            ref = c["ref"][name]
            assert float((got - ref).abs().max()) <= 1e-11 * max(1.0, float(ref.abs().max())), (what, name)
        count += 1
    assert count > 50
    for M, C in bu.STATS_CASES:            # the statistics and the running buffers
        c = bu.stats_case(M, C)
        rm, rv = bu._t(c["rm0"], torch.float64).clone(), bu._t(c["rv0"], torch.float64).clone()
        x = bu._t(c["y"], torch.float64)
        F.batch_norm(x, rm, rv, None, None, True, bu.MOMENTUM, bu.EPS_BN)
        assert torch.allclose(rm, c["ref"]["rmean"], rtol=1e-12, atol=1e-13) and torch.allclose(rv, c["ref"]["rvar"], rtol=1e-12, atol=1e-13)
        assert torch.allclose(x.mean(0), c["ref"]["mean"], rtol=1e-12, atol=1e-13)
        assert torch.allclose(1 / torch.sqrt(x.var(0, unbiased=False) + bu.EPS_BN), c["ref"]["rstd"], rtol=1e-12)


def test_partial_rows_give_the_statistics_of_their_matrix():
    for R in bu.PARTIALS_R:
        for C in bu.PARTIALS_C:
            c = bu.partials_case(R, C)
            assert c["part"].shape == (R, 2, C) and c["M"] == 64 * R
            y = bu.ofill.fill(f"bnpool/partials/{R}x{C}/y", (64 * R, C), std=1.0, mean=0.3).astype(np.float64)
            assert np.allclose(c["ref"]["mean"].numpy(), y.mean(0), rtol=1e-6, atol=1e-7)
            assert np.allclose(c["ref"]["rstd"].numpy(), 1 / np.sqrt(y.var(0) + bu.EPS_BN), rtol=1e-6)


def test_fp32_and_fp64_pick_the_same_winners_and_signs():
    """the input condition: no window whose winner, and no element whose LeakyReLU branch, fp32 and fp64 decide differently --
    zero disagreements in every case; and the ties the cases are built for are there"""
    for what, c in bu.all_act_cases():
        ref, got = c["ref"], c["got32"]
        assert torch.equal(ref["idx"], got["idx"]), (what, int((ref["idx"] != got["idx"]).sum()))
        assert torch.equal(torch.sign(ref["z"]), torch.sign(got["z"]).double()), what
        assert np.array_equal(c["y"] * bu.GRID, np.round(c["y"] * bu.GRID))
        if c["gamma"] is not None:
            g, b = c["gamma"], c["beta"]
            assert (g > 0).any() and (g < 0).any() and (g == 0).any() and np.abs(g[g != 0]).min() >= 0.5
            zero = np.flatnonzero(g == 0)
            assert (b[zero] == 0).any()
            # gamma == 0: the whole window ties and its first tap inside the map wins; z == 0 exactly where beta is 0 too
            first = ref["idx"][..., zero].reshape(-1, len(zero)).max(0).values
            k = c["pool"][1]
            pad = 0 if c["pool"][0] == "win" else c["pool"][3]
            assert int(first.max()) <= pad * k + pad, what
            assert bool((ref["z"][..., zero[b[zero] == 0]] == 0).all())
        if c["slope"] == 0.0 and c["pool"][1] > 1:
            assert float((ref["out"] == 0).double().mean()) > 0.02, what          # windows that tie at 0


def test_fp32_cpu_evaluation_stays_within_every_bound():
    count = 0
    for what, ref, got32, specs in bu.all_measured_cases():
        names = [k for k in specs if k in got32 and k in ref]
        bu.compare(what, got32, ref, specs, names, verbose=False)
        count += 1
    for what, c in bu.all_act_cases():
        specs = bu.act_specs(c)
        bu.compare(str(what), c["got32"], c["ref"], specs, ("out", "flat", "dy", "dgamma", "dbeta"), verbose=False)
        count += 1
    assert count > 150


def test_measured_constants_are_the_reference_errors():
    """REF_ERR32 holds what the fp32-CPU evaluation measures: never below it, and not inflated past it (the bound then adds the
    factor K_KERNEL and the floor, nothing else)"""
    table = bu.measure()
    assert set(table) == set(bu.REF_ERR32)
    for key, got in table.items():
        assert got <= bu.REF_ERR32[key] <= 2.0 * got + bu.ULP32, (key, got, bu.REF_ERR32[key])
    assert bu.K_KERNEL == 4.0 and bu.FLOOR_ULPS <= 4.0
    assert bu.TOL_BN_FWD == (1e-4, 1e-4) and bu.TOL_BN_GRAD == (1e-3, 1e-4)
    assert bu.tol16(bu.TOL_BN_GRAD, torch.bfloat16) == (1e-3 + 2.0 ** -7, 1e-4)


def test_statistics_cases_reach_their_launch_paths():
    launch = {mc: bu.stats_launch(*mc) for mc in bu.STATS_CASES}
    assert all(launch[(37, C)][0] == 1 for C in (1, 3, 5))                                     # VEC = 1
    assert launch[(2, 4)][1] == 1 and launch[(300, 4)][1] == 1                                 # cpb = 1: fewer / more rows than threads
    for M in (1023, 1024, 1025):           # the four-loads-in-flight loop: step = gy * rpb rows, 4 steps an iteration
        vec, cpb, gx, gy, _, _ = launch[(M, 64)]
        assert vec == 4 and M >= 4 * gy * (256 // cpb)
    step = launch[(1024, 64)][3] * (256 // launch[(1024, 64)][1])
    assert 1024 % (4 * step) == 0 and 1023 % (4 * step) != 0                                   # exactly full iterations / a tail
    assert launch[(33000, 256)][5] and not launch[(33000, 256)][4]                             # gy > 512
    assert launch[(4200, 4096)][4] and launch[(4200, 4096)][2] > 1                             # gx * gy > 1024
    assert launch[(500, 20)][0] == 4 and 20 % 16 != 0
    c = bu.stats_case(*bu.STATS_BIGMEAN, bigmean=True)
    ratio = c["ref"]["mean"] * c["ref"]["rstd"]
    assert float(ratio.min()) > 7.5 and float(ratio.max()) < 8.5                               # mean = 8 x std
    assert set(bu.PARTIALS_R) == {1, 63, 1024, 1025, 2049, 3000} and set(bu.PARTIALS_C) == {4, 20}


def test_backward_cases_reach_their_launch_paths():
    cases = bu.bwd_cases()
    by_q = {}
    for a in cases:
        n, H, W, C, P = a[:5]
        items, q, g0, grid = bu.bwd_launch(n, H, W, C, P)
        by_q.setdefault(q if C != 64 else "big", []).append((a, items, g0, grid))
    assert set(by_q) == {1, 3, 5, 257, 1023, 4, "big"}
    for q, lst in by_q.items():
        if q == "big":
            continue
        # every option meets every q class: (P, flat, dy dtype, training, accumulate, dgb, y dtype)
        for pos, values in ((4, {1, 2}), (5, {0, 1}), (7, {True, False}), (8, {0, 1}), (9, {True, False})):
            assert {a[pos] for a, *_ in lst} == values, (q, pos)
        assert {a[6] is None for a, *_ in lst} == {True, False} and {a[10] is None for a, *_ in lst} == {True, False}
        assert {a[11] for a, *_ in lst} == {0.0, 0.01}
    # every instantiation P x YT runs
    assert {(a[4], a[10]) for a in cases} == {(P, yd) for P in (1, 2) for yd in (None,) + bu.DTYPES}
    assert any(items < 256 and g0 == 1 for _, items, g0, _ in by_q[1])                         # one partly idle workgroup
    assert any(items < 256 and g0 == 3 for _, items, g0, _ in by_q[3])                         # ... and q - 1 empty ones
    assert any(items > g0 * 256 and items % (g0 * 256) for _, items, g0, _ in by_q[5])         # no multiple of the grid stride
    assert any((grid * 256) % 5 for _, _, _, grid in by_q[5])                                  # the apply pass reloads its quad
    assert all(g0 == 257 and items < 257 * 256 for _, items, g0, _ in by_q[257])               # whole idle workgroups
    assert all(g0 == 1023 for _, _, g0, _ in by_q[1023]) and all(g0 % 4 == 0 for _, _, g0, _ in by_q[4])
    (a, items, g0, grid), = by_q["big"]
    assert a[:4] == (9, 64, 60, 64) and items > 2 * 1024 * 256 and g0 == 1024
    assert all(a[1] != a[2] for a in cases if a[3] != 4092)                                    # non-square maps


def test_pooling_cases_reach_their_paths():
    s2k3 = [bu.is_s2k3(*g) for g in bu.MAXPOOL_GEOS]
    assert s2k3 == [True, False, False, False, False, False]
    assert [g[1] for g in bu.MAXPOOL_GEOS] == [2, 2, 2, 1, 3, 2] and all(g[3] != g[4] for g in bu.MAXPOOL_GEOS)
    for gi, C in ((2, 12), (4, 12)):       # pixels that fall in no window, or between windows: no upstream gradient, yet
        for training in (True, False):     # the BatchNorm mean terms reach them when training, and exactly 0 in eval
            c = bu.maxpool_case(gi, C, training)
            un = bu.unwon_pixels(c)
            live = torch.from_numpy(c["gamma"] != 0)
            assert bool(un[:, -1 if gi == 2 else 2].all())
            dy = c["ref"]["dy"].reshape(un.shape)
            if training:
                assert bool((dy[un & live] != 0).all())
            else:
                assert bool((dy[un] == 0).all())
    for gi in range(len(bu.MAXPOOL_GEOS)):
        assert {bu.maxpool_slope(gi, ci) for ci in range(len(bu.MAXPOOL_C))} == {0.0, 0.01}
    assert set(bu.FWD_SLOPES) == {0.0, 0.01, 1.0}
    fc = bu.fwd_cases()
    for key in (3, 4, 7):                  # every slope meets every C, pool and y type
        for v in {a[key] for a in fc}:
            assert {a[5] for a in fc if a[key] == v} == set(bu.FWD_SLOPES), (key, v)
    assert any(not a[6] for a in fc) and {a[:3] for a in fc} == set(bu.FWD_SHAPES)
    assert set(bu.COLSUM_C) == {4, 1028, 4092} and set(bu.COLSUM_ROWS) == {1, 3, 70000}
    assert bu.JUNCTION_COUNTS[2] // 4 == bu.JUNCTION_GRID_CAP * 256 + 1
    for count in bu.JUNCTION_COUNTS[:2]:
        c = bu.junction_case(count)
        s = c["a"] + c["b"]
        assert (s == 0).any() and np.signbit(c["a"][1]) and np.signbit(c["b"][1]) and (s > 0).any() and (count == 4 or (s < 0).any())
    for n, HW, C in bu.AVGPOOL_CASES:
        cpb = min(C // 4, 64)
        assert C % 16 == 0 and 256 % cpb == 0 and (C // 4) % cpb == 0
    for C in bu.AVGPOOL_REFUSED_C:
        cpb = min(C // 4, 64)
        assert C % 16 or 256 % cpb or (C // 4) % cpb
    x = bu.avgpool_case(2, 1000, 512)["x"]
    assert ((x == x.max(1, keepdims=True)).sum(1) > 1).any()                                   # columns whose maximum ties
