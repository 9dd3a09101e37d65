"""The references, input conditions and tolerance table of the CBAM gate kernel tests (tests/cbam_util.py), checked without a GPU: the
hand-written restatement agrees with the oracle modules under fp64 autograd, fp32 and fp64 pick the same argmax_c, argmax_p and ReLU
masks in every case (zero exceptions) and the planted ties are there, the measured constants are what the fp32-CPU evaluation
gives, and the case tables reach the launch paths they claim."""
import numpy as np
import torch

import cbam_util as cu


def test_restatement_agrees_with_the_oracle_modules_under_autograd():
    """out, dx, g, the seven parameter gradients and the running buffers of every case below a million elements; the record, datt and
    the slices are intermediate values of that same backward: the slices add up to the full sum datt is made of"""
    count = 0
    for what, c in cu.all_cases(heavy=False):
        r, a = cu.restate(c, torch.float64), cu.autograd(c, torch.float64)
        for name, want in a.items():
            if name == "nbt":
                assert want == cu.NBT0 + (1 if c["training"] else 0), what
                continue
            got, want = cu._np64(r[name]).reshape(want.shape), cu._np64(want)
            assert float(np.abs(got - want).max()) <= 1e-11 * max(1.0, float(np.abs(want).max())), (what, name)
        if c["part"] == "fused":
            assert r["slices"].shape[0] == c["nz"]
            sc = r["scale"]
            assert torch.allclose(r["slices"].sum(0) * sc * (1 - sc), r["datt"], rtol=1e-12, atol=1e-14), what
            per = -(-c["H"] * c["W"] // c["nz"])
            assert per * (c["nz"] - 1) < c["H"] * c["W"]                                  # no empty slice
        count += 1
    assert count > 70


def test_fp32_and_fp64_pick_the_same_winners_and_masks():
    """the input condition, over every case: zero disagreements in argmax_c, argmax_p, hidden > 0 and out > 0; the first maximum is
    numpy's argmax of the grid input; the planted ties are where the module docstring says"""
    for what, c in cu.all_cases():
        ref, got, x = c["ref"], c["got32"], c["x"]
        n, HW, C = x.shape
        assert np.array_equal(x * 64.0, np.round(x * 64.0)) and (c["res"] is None or np.array_equal(c["res"] * 64.0, np.round(c["res"] * 64.0)))
        for k in ("argmax_c", "argmax_p"):
            if k in ref:
                assert torch.equal(ref[k], got[k]), (what, k, int((ref[k] != got[k]).sum()))
        if "hidden" in ref:
            assert torch.equal(ref["hidden"] > 0, got["hidden"] > 0), what
        assert torch.equal(ref["out"] > 0, got["out"] > 0), what
        if c["res"] is not None:
            assert 0.05 < float((ref["out"] > 0).double().mean()) < 0.95, what             # both branches of the junction's ReLU
        if c["part"] != "sgate":
            am = ref["argmax_c"].numpy()
            assert np.array_equal(am, x.argmax(1)), what
            assert (x[0, :, 0] == 0).all() and am[0, 0] == 0                              # a constant plane: position 0
            if HW >= 3:
                rpb = 256 // cu.chan_cpb(C)
                hits = np.flatnonzero(x[n - 1, :, 1] == cu.BIG)
                assert len(hits) == 2 and hits[0] % rpb != hits[1] % rpb and am[n - 1, 1] == hits[0] == 1, what
        if c["part"] == "sgate":
            am = ref["argmax_p"].numpy()
            assert np.array_equal(am, x.argmax(2)), what
        if c["part"] != "cgate" and HW >= 4:
            am = ref["argmax_p"].numpy()
            assert (x[n - 1, 0] == 0).all() and am[n - 1, 0] == 0, what                   # a pixel of equal channels: channel 0
            hw = HW // 2
            if C >= 8 and c["part"] == "sgate":
                tied = np.flatnonzero(x[0, hw] == cu.BIG)
                assert len(tied) >= 2 and len({(t // 4) % 16 for t in tied.tolist()}) >= 2 and am[0, hw] == tied[0], what
                assert C < 128 or {2, 66} <= set(tied.tolist())                           # the same sub-lane's second round


def test_fp32_cpu_evaluation_stays_within_every_bound():
    count = 0
    for what, c in cu.all_cases():
        names = [k for k in c["specs"] if k in c["got32"] and k in c["ref"]]
        assert {"out", "dx"} <= set(names)
        cu.compare(what, c["got32"], c["ref"], c["specs"], names, verbose=False)
        count += 1
    assert count > 80


def test_measured_constants_are_the_reference_errors():
    """REF_ERR32 holds what the fp32-CPU evaluation measures: never below it, and not inflated past it"""
    table = cu.measure()
    assert set(table) == set(cu.REF_ERR32)
    for key, got in table.items():
        assert got <= cu.REF_ERR32[key] <= 2.0 * got + cu.ULP32, (key, got, cu.REF_ERR32[key])
    assert cu.K_KERNEL == 4.0 and cu.FLOOR_ULPS <= 4.0
    assert cu.TOL_Y == (1e-4, 1e-5) and cu.TOL_DX == (1e-3, 1e-4) and cu.TOL_PGRAD == 2e-4


def test_case_tables_reach_their_paths():
    # channel gate: the refused lists are exactly what chan_cpb's arithmetic refuses; every table entry is accepted
    for C in cu.CGATE_REFUSED_C:
        assert not cu.cgate_accepts(C, 4)
    for Ch in cu.CGATE_REFUSED_CH:
        assert cu.cgate_accepts(64, 4) and not cu.cgate_accepts(64, Ch)
    cpb = {C: cu.chan_cpb(C) for C in cu.CGATE_REFUSED_C}
    assert 256 % cpb[48] and 256 % cpb[80] and 256 % cpb[96] and (320 // 4) % cpb[320] and 8 < 16 and 4112 > 4096
    for n, H, W, C, Ch in cu.CGATE_CASES + cu.FUSED_CASES + (cu.FUSED_DATA_ONLY,):
        assert cu.cgate_accepts(C, Ch), C
    rpb = {C: 256 // cu.chan_cpb(C) for C in (16, 32, 64, 256, 4096)}
    assert rpb == {16: 64, 32: 32, 64: 16, 256: 4, 4096: 4}
    hw = {(C, H * W) for _, H, W, C, _ in cu.CGATE_CASES}
    assert {(16, 1), (16, 63), (16, 64), (16, 65)} <= hw and {(64, 127), (64, 128), (64, 129)} <= hw and 8 * rpb[64] == 128
    assert (256, 3) in hw and 3 < rpb[256] and (4096, 4) in hw
    assert {Ch for *_, Ch in cu.CGATE_CASES} >= {1, 3, 256} and {n for n, *_ in cu.CGATE_CASES} >= {1, 17, 70}
    # spatial gate
    shapes = cu.SGATE_SMALL + cu.SGATE_LARGE
    assert all(cu.sgate_bwd_accepts(H, W) for _, H, W, _ in shapes) and not cu.sgate_bwd_accepts(*cu.SGATE_REFUSED_BWD[1:3])
    assert (58 + 6) * (122 + 6) == 8192 and (2, 58, 122, 4) in shapes
    assert cu.plane_exceeds_stage(84, 84) and cu.plane_exceeds_stage(74, 74) and not cu.plane_exceeds_stage(73, 74)
    assert any(H < 7 < W for _, H, W, _ in shapes) and any(W < 7 < H for _, H, W, _ in shapes) and any(C % 64 for *_, C in shapes if C > 64)
    assert any(n > 64 for n, *_ in shapes)
    n, H, W, C = cu.SGATE_LARGE[-1]
    P = n * H * W
    assert P > 8192 * 256 and P > 8192 * 16 and P * C // 4 > 8192 * 256 and P > 512 * 256  # a second round everywhere, all 512 partials
    # fused unit: the table as a whole reaches every nz
    nz = {a: cu.junction_nz(a[0], a[1] * a[2], a[3]) for a in cu.FUSED_CASES}
    assert set(nz.values()) == {1, 2, 4, 8}
    assert nz[(2, 8, 16, 64, 4)] == 2 and nz[(2, 16, 16, 64, 4)] == 4 and nz[(2, 32, 32, 64, 4)] == 8 and nz[(1, 56, 56, 64, 4)] == 8
    assert nz[(2, 31, 33, 64, 4)] == 8 and (31 * 33) % 8 and -(-31 * 33 // 8) * 7 < 31 * 33                # a short last slice
    assert nz[(300, 16, 32, 16, 1)] == 4 and cu.junction_nz(2, 16 * 32, 16) == 8                        # n limits nz
    assert 45 * 56 * 56 > 8192 * 16
    assert not cu.sgate_bwd_accepts(*cu.FUSED_DATA_ONLY[1:3])
    for what, c in cu.all_cases(heavy=False):
        if c["part"] == "fused":
            assert c["nz"] == nz.get((c["n"], c["H"], c["W"], c["C"], c["Ch"]), 8 if (c["H"], c["W"]) == (58, 123) else None), what
