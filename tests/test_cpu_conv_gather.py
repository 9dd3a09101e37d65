"""No GPU: the tables and references of tests/conv_gather_util.py are fit for a bitwise comparison (its docstring) -- the exactness
condition holds for every case, the unfold is the convolution of torch in fp64, every mutant changes every case it applies to and every
kernel has a case for every mutant of its family, the restated gather routes are the dispatcher's at 64 to 304 CUs, and the entry points
refuse what they cannot address (the checks that return before any HIP call)."""
import numpy as np
import pytest
import torch

import conv_gather_util as u

CU_COUNTS = (64, 80, 104, 128, 228, 256, 304)


@pytest.fixture(scope="module")
def lib():
    from eoe_amd import _lib
    return _lib


def test_exactness_condition_holds_for_every_case_of_every_table():
    """the sum of |terms| of every accumulator < 2^24 (inputs are dtype-independent integers, exact in bf16 and fp16 alike)"""
    assert u.exactness_failures() == []
    for c in u.nt_cases(heavy=False) + u.tn_table():
        x = (u.nt_inputs if "kernel" in c else u.tn_inputs)(c)
        for n in ("a", "b"):
            for dt in u.DTYPES:
                assert np.array_equal(u.t16(x[n], dt).double().numpy(), x[n]), (c["id"], n)
    code = u.position_code("t", (3, 5, 7, 8))
    assert np.abs(code).min() >= 1 and np.abs(code).max() <= 120 and len(np.unique(code)) > 200


def _all_geometries():
    gs = [(u.geo(n, 2), 5) for n in u.GEOS]
    gs += [(u.stem_geo(*s, 2)["g2"], 4) for s in u.STEMS]
    return gs


@pytest.mark.parametrize("g,Cc", _all_geometries(), ids=lambda v: v["name"] if isinstance(v, dict) else str(v))
def test_unfold_is_the_convolution_of_torch_in_fp64(g, Cc):
    x = u.ints("conv2d/x/" + g["name"], (g["n"], g["H"], g["W"], Cc))
    w = u.ints("conv2d/w/" + g["name"], (6, Cc, g["kh"], g["kw"]))
    got = u.unfold(x, g) @ w.transpose(0, 2, 3, 1).reshape(6, -1).T
    ref = torch.nn.functional.conv2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), torch.from_numpy(w).double(), stride=g["s"], padding=g["p"])
    ref = ref[:, :, :g["Ho"], :g["Wo"]]                           # (the packed first layer's grid may stop short of the padded image)
    assert ref.shape[2:] == (g["Ho"], g["Wo"])
    assert np.array_equal(got.reshape(g["n"], g["Ho"], g["Wo"], 6), ref.permute(0, 2, 3, 1).numpy())
    # and its transpose (col2im) against the convolution's input gradient
    dy = u.ints("conv2d/dy/" + g["name"], (g["n"] * g["Ho"] * g["Wo"], 6))
    dx = u.col2im_ref(dy @ w.transpose(0, 2, 3, 1).reshape(6, -1), g, Cc)[0]
    xr = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_()
    out = torch.nn.functional.conv2d(xr, torch.from_numpy(w).double(), stride=g["s"], padding=g["p"])[:, :, :g["Ho"], :g["Wo"]]
    out.backward(torch.from_numpy(dy).double().reshape(g["n"], g["Ho"], g["Wo"], 6).permute(0, 3, 1, 2))
    assert np.array_equal(dx, xr.grad.permute(0, 2, 3, 1).numpy())


def test_every_mutant_changes_every_nt_case_it_applies_to_and_every_kernel_meets_every_mutant():
    missing, same = [], []
    for kernel, cases in u.nt_table().items():
        assert all(c["expect"] == kernel for c in cases), kernel                 # at 256 CUs nothing skips
        for mutant in u.kernel_mutants(kernel):
            hit = False
            for c in cases:
                if not u.applies(mutant, c["gg"], c["C"], Kp=c["K"]):
                    continue
                hit = True
                rows = u.case_rows(c)
                code = u.probe_activation(c)
                if np.array_equal(u.nt_patch(c, code, rows, mutant), u.nt_patch(c, code, rows)):
                    same.append((c["id"], mutant, "probe"))
                if np.array_equal(u.nt_expected(c, rows, mutant)["C"], u.nt_expected(c, rows)["C"]):
                    same.append((c["id"], mutant, "arithmetic"))
            if not hit:
                missing.append((kernel, mutant))
    assert not missing, f"kernels without a case for a mutant: {missing}"
    assert not same, f"cases a mutant does not change: {same}"


def test_every_mutant_changes_every_tn_case_it_applies_to():
    same, met = [], {1: set(), 2: set()}
    for c in u.tn_table():
        for mutant in (u.GATHER_MUTANTS if c["mode"] == 1 else u.STEM_MUTANTS):
            if not u.applies(mutant, c["gg"], c["C"]):
                continue
            met[c["mode"]].add(mutant)
            code = u.probe_activation(c)
            if np.array_equal(u.unfold(code, c["gg"], mutant=mutant), u.unfold(code, c["gg"])):
                same.append((c["id"], mutant, "probe"))
            if np.array_equal(u.tn_expected(c, mutant=mutant)["C"], u.tn_expected(c)["C"]):
                same.append((c["id"], mutant, "arithmetic"))
    assert met[1] == set(u.GATHER_MUTANTS) and met[2] == set(u.STEM_MUTANTS), met
    assert not same, same
    # the split forms: with and without a workspace, unpack_dw, accumulate, and a split boundary inside an image, at every CU count
    for ncu in CU_COUNTS:
        for c in u.tn_table():
            s, t_per = u.tn_splits(c, ncu)
            assert (s >= 2) == c["split"], (c["id"], ncu)
            if c["split"]:
                assert t_per % (c["gg"]["Ho"] * c["gg"]["Wo"]) != 0, c["id"]
    split = [(c["ws"], c["accumulate"]) for c in u.tn_table() if c["split"]]
    assert {("ws", False), ("ws", True), ("unpack", False), ("unpack", True), ("none", False), ("none", True)} <= set(split)


def test_pack_and_im2col_tables_tell_their_mutants():
    """the pack kernels' family: kx_major, taps_reversed, c_mod_cpad, tail_nonzero -- each changes some output of every job it applies to"""
    met = set()
    for j in u.pack_jobs(33):
        taps = j["kh"] * j["kw"]
        ref = u.pack_ref(j["w"], j["cpad"], j["Kp"])
        for mutant, on in (("kx_major", j["kh"] > 1 and j["kw"] > 1), ("taps_reversed", taps > 1), ("c_mod_cpad", taps > 1),
                           ("tail_nonzero", j["Kp"] > taps * j["cpad"])):
            if on:
                met.add(mutant)
                got = u.pack_ref(j["w"], j["cpad"], j["Kp"], mutant)
                assert any(not np.array_equal(a, b) for a, b in zip(got, ref)), (j["cout"], j["cin"], j["kh"], j["kw"], mutant)
    assert met == {"kx_major", "taps_reversed", "c_mod_cpad", "tail_nonzero"}
    assert {(bool(j["t"]), bool(j["d"])) for j in u.pack_jobs(33)} == {(True, True), (True, False), (False, True), (False, False)}
    met = set()
    for r in u.im2col_cases():
        x = u.position_code(r["id"], (r["g"]["n"], r["g"]["H"], r["g"]["W"], r["cin"]))
        for mutant in u.MUTANTS:
            if u.applies(mutant, r["g"], r["cin"], Kp=r["Kp"]):
                met.add((r["kind"], mutant))
                assert not np.array_equal(u.unfold(x, r["g"], Kp=r["Kp"], mutant=mutant), u.unfold(x, r["g"], Kp=r["Kp"])), (r["id"], mutant)
    assert met == {(k, m) for k in (0, 1, 2) for m in u.MUTANTS}
    # col2im: the transpose of the same unfold; strides 1, 2 and the run-time 3, the 1-wide maps, both accumulate values
    cs = u.col2im_cases()
    assert {r["g"]["s"] for r in cs} == {1, 2, 3} and {r["C"] for r in cs} == {4, 12, 64} and {r["accumulate"] for r in cs} == {0, 1}
    assert any(r["g"]["W"] == 1 for r in cs) and any(r["g"]["H"] == 1 for r in cs)


def test_tables_reach_the_edges_the_kernels_have():
    t = u.nt_table()
    for kernel, cases in t.items():
        tile = u.KERNELS[kernel][2]
        assert any(c["M"] > tile and tile % (c["gg"]["Ho"] * c["gg"]["Wo"]) != 0 for c in cases), f"{kernel}: no M tail in another image"
        assert all(c["form"] == u.KERNELS[kernel][1] for c in cases)
        if not kernel.startswith("nt128_mi5"):
            assert any(c["ldc"] > c["N"] for c in cases) and any(c["ldc"] == c["N"] for c in cases), kernel
    for kernel in ("pers_ni2_g3", "pers_ni4_g3"):
        cs = [c for c in t[kernel] if not c["heavy"]]
        assert {(c["C"], c["gg"]["kh"]) for c in cs} >= {(C_, k) for C_ in (8, 16, 32) for k in (3, 5)}
        assert any(c["K"] == c["Kmin"] for c in cs) and any(c["K"] - c["Kmin"] >= 64 for c in cs) and any(0 < c["K"] - c["Kmin"] < 64 for c in cs)
    assert {(c["g"]["kh"] % 2, c["g"]["s"]) for c in t["nt64_g2"]} == {(0, 2), (1, 2), (1, 4)}
    assert {c["g"]["kh"] for c in t["nt64_g2"]} == {3, 7, 8} and {c["g"]["kw"] for c in t["nt64_g2"]} == {3, 7, 8}
    for kernel in ("pers_ni4_g1", "pers_ni4_g2", "pers_ni4_g3"):                  # a second tile per workgroup at every CU count
        for ncu in CU_COUNTS:
            heavy = [c for c in u.nt_table(ncu)[kernel] if c["heavy"]]
            assert len(heavy) == 1 and u.cdiv(heavy[0]["M"], 256) * u.cdiv(heavy[0]["N"], 128) > ncu and heavy[0]["gg"]["kh"] >= 2
    kinds = {c["kind"] for c in u.nt_cases()}
    assert kinds == set(u.KINDS)
    assert any(c["gg"]["kh"] != c["gg"]["kw"] for c in u.nt_cases() if c["mode"] != 2) and any(c["gg"]["kh"] != c["gg"]["kw"] for c in u.tn_table())


@pytest.mark.parametrize("ncu", CU_COUNTS)
def test_restated_gather_routes_are_the_dispatchers(lib, ncu):
    """eoe_gemm_nt_route accepts every case (fill_params' geometry checks included) and names the gather route; the restatement sends every
    case to the kernel it is for.  (Which of the six kernels runs is `nt_last_form`, asserted per launch on the GPU.)"""
    for kernel, cases in u.nt_table(ncu).items():
        for c in cases:
            assert c["expect"] == kernel or kernel == "nt128_mi5", (c["id"], c["expect"])
            for dt in u.DTYPES:
                old = lib.set_option("nt_flags", c["flags"])
                try:
                    assert lib.gemm_nt_route(u.nt_args(c, dt, u.fake_addr(c)), ncu) == lib.NT_KERNEL_GATHER, c["id"]
                finally:
                    lib.set_option("nt_flags", old)
    assert lib.get_option("nt_last_form") == 0 or ncu                             # the option exists; nothing was launched here


def _tn_rc(lib, args, count=1):
    return lib.lib.eoe_gemm_tn_grouped(args, count, None)


def _tn_fake(lib, g, Cc, M, N, mode=1):
    T = g["n"] * g["Ho"] * g["Wo"]
    a = lib.GemmArgs(1 << 32, 2 << 32, 3 << 32, None, None, None, None, M, N, T, 0, N, N, 0, lib.EOE_F16, 0, 1, 0, 1.0)
    a.gather, a.geo = mode, u.geometry(g, Cc)
    return a


def test_tn_gather_refuses_what_it_cannot_decode(lib):
    """all of these return from the argument checks, before any HIP call"""
    g = u.geo("3s1_9x7", 2)

    def refused(args, what, count=1):
        arr = (lib.GemmArgs * count)(*([args] * count))
        assert _tn_rc(lib, arr, count) != 0
        assert what in lib.lib.eoe_last_error().decode(), lib.lib.eoe_last_error()

    refused(_tn_fake(lib, g, 8, 72, 8), "cannot be grouped", count=2)
    refused(_tn_fake(lib, g, 8, 80, 8), "does not match M")
    refused(_tn_fake(lib, u.geo("2x3s1_7x9", 2), 12, 72, 8), "does not match M")                                        # C % 8
    big = dict(g, n=1, H=256, W=256, Ho=256, Wo=256)
    refused(_tn_fake(lib, big, 8, 72, 8), "bad conv geometry")                                      # Ho Wo >= 65536
    refused(_tn_fake(lib, dict(g, n=258, H=255, W=256, Ho=255, Wo=256), 8, 72, 8), "bad conv geometry")        # T >= 2^24
    s = u.stem_geo(3, 7, 2, 1, 10, 13, 2)
    refused(_tn_fake(lib, dict(s["g2"], H=s["g2"]["H"] - 2), 4, 128, 8, mode=2), "packed first-layer")          # the window leaves the image
    refused(_tn_fake(lib, dict(s["g2"], W=s["g2"]["W"] - 2), 4, 128, 8, mode=2), "packed first-layer")
    refused(_tn_fake(lib, s["g2"], 4, 64, 8, mode=2), "packed first-layer")                                   # M != ceil(kh/2) 64


def test_nt_gather_refuses_what_it_cannot_decode(lib):
    c = u.nt_table()["nt64_g1"][0]

    def refused(c2, what):
        with pytest.raises(lib.EoeError, match=what):
            lib.gemm_nt_route(u.nt_args(c2, torch.float16, u.fake_addr(c2)), 256)

    refused(dict(c, C=24), "bad conv geometry")                                      # neither 8, 16, 32 nor a multiple of 64
    refused(dict(c, K=c["K"] + 64, ldb=c["K"] + 64), "does not match")                               # mode 1: K == kh kw C
    refused(dict(c, M=c["M"] + 1), "does not match")
    n3 = u.nt_table()["pers_ni2_g3"][0]
    refused(dict(n3, K=n3["K"] - 64), "does not match")                             # narrow: K >= kh kw C
    s = u.nt_table()["nt64_g2"][0]
    refused(dict(s, gg=dict(s["gg"], H=s["gg"]["H"] - 2)), "image must be padded")
    refused(dict(s, gg=dict(s["gg"], W=s["gg"]["W"] - 1)), "packed first-layer")     # W odd
    refused(dict(s, gg=dict(s["gg"], s=3)), "packed first-layer")                    # odd stride


def _store(c, dtype, mem, exact, ld_rows_cols):
    rows, cols, ld = ld_rows_cols
    out16 = "kernel" in c and u.kind_of(c)["out"] == "16"
    val = u.rne16(exact, dtype) if out16 else torch.from_numpy(exact.astype(np.float32))
    u.gu.view_of(mem["C"][0], rows, cols, ld, mem["C"][1]).copy_(val.reshape(rows, cols))


@pytest.mark.parametrize("dtype", u.DTYPES, ids=lambda d: u.DTNAME[d])
def test_comparison_functions_accept_the_reference_and_reject_a_mutant_and_a_stray_store(dtype):
    """what the GPU tier calls after a launch, fed on the CPU: the exact result passes, one wrong tap or one store outside the view fails"""
    for kernel, cases in u.nt_table().items():
        c = next(c for c in cases if not c["heavy"]) if any(not c["heavy"] for c in cases) else None
        if c is None:
            continue
        stats = torch.from_numpy(u.nt_expected(c)["stats"].astype(np.float32)) if u.kind_of(c)["colstats"] else None
        view = (c["M"], c["N"], c["ldc"])
        mem = u.nt_memory(c, dtype)
        _store(c, dtype, mem, u.nt_expected(c)["C"], view)
        assert u.nt_failures(c, dtype, mem, stats) == [], c["id"]
        mutant = next(m for m in u.kernel_mutants(kernel) if u.applies(m, c["gg"], c["C"], Kp=c["K"]))
        _store(c, dtype, mem, u.nt_expected(c, mutant=mutant)["C"], view)
        assert any(f.startswith("bits:C") for f in u.nt_failures(c, dtype, mem, stats)), (c["id"], mutant)
        _store(c, dtype, mem, u.nt_expected(c)["C"], view)
        mem["C"][0][mem["C"][1] - 1] = 1.0
        assert any(f.startswith("canary:C") for f in u.nt_failures(c, dtype, mem, stats)), c["id"]
        if stats is not None:
            stats[-1, 1, 0] += 1
            mem = u.nt_memory(c, dtype)
            _store(c, dtype, mem, u.nt_expected(c)["C"], view)
            assert any(f.startswith("bits:colstats") for f in u.nt_failures(c, dtype, mem, stats)), c["id"]
    for c in u.tn_table()[::4]:
        mem = u.tn_memory(c, dtype)
        _store(c, dtype, mem, u.tn_expected(c)["C"], u.tn_out_view(c))
        assert u.tn_failures(c, mem, 256) == [], c["id"]
        _store(c, dtype, mem, u.tn_expected(c, mutant="hw_swapped")["C"], u.tn_out_view(c))
        assert u.tn_failures(c, mem, 256) != [], c["id"]
