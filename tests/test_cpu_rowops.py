"""The tolerance table and the case tables of the row-kernel tests (tests/rowops_util.py), checked without a GPU: the oracle's
fp32-CPU evaluation of every case stays inside the bound its kernel gets, the measured constants are what this evaluation gives,
the edge logits keep clear of the focal clamp edges, and no table lost a listed size."""
import numpy as np
import torch

import rowops_util as ru
from oracle import objectives as oobj


def test_fp32_cpu_evaluation_stays_within_every_bound():
    count = 0
    for what, ref, got32, specs in ru.all_cases():
        ru.compare(what, got32, ref, specs, verbose=False)
        count += 1
    assert count > 400


def test_measured_constants_are_the_reference_errors():
    """REF_ERR32 holds what the fp32-CPU evaluation measures: never below it, and not inflated past it (the bound then adds the
    factor K_KERNEL and the floor, nothing else)"""
    table = ru.measure()
    assert set(table) == set(ru.REF_ERR32)
    for key, got in table.items():
        assert got <= ru.REF_ERR32[key] <= 2.0 * got + ru.ULP32, (key, got, ru.REF_ERR32[key])
    assert ru.K_KERNEL == 4.0 and ru.FLOOR_ULPS <= 4.0


def test_edge_logits_keep_clear_of_the_focal_clamp_edges():
    x, y = ru.edge_logit_table()
    assert set(np.abs(x).tolist()) == {0.0, np.float32(1e-4), 5.0, 17.0, 40.0, 90.0, 200.0} and set(y.tolist()) == {0, 1}
    assert (ru.focal_edge_distance(x, y) > 1e-3).all()
    # fp32 and fp64 agree on which side of each edge every logit falls, and all three regions are hit by both labels
    sides = []
    for dt in (torch.float64, torch.float32):
        raw = torch.exp(-oobj.bce_losses(torch.from_numpy(x).to(dt), torch.from_numpy(y)))
        sides.append(np.where(raw.numpy() < ru.FOCAL_EPS, -1, np.where(raw.numpy() > 1.0 - ru.FOCAL_EPS, 1, 0)))
    assert (sides[0] == sides[1]).all()
    for label in (0, 1):
        assert set(sides[0][y == label].tolist()) == {-1, 0, 1}
    c = ru.elem_case("focal", 0, "edge")
    for k in ("rows", "grad", "loss"):
        assert torch.isfinite(c["got32"][k]).all() and torch.isfinite(c["ref"][k]).all()


def test_case_tables_cover_the_listed_sizes():
    assert ru.LN_MANY == ((9000, 256), (4100, 1024)) and ru.LN_INST == (33, 512) and ru.LN_BIGMEAN == (64, 768)
    assert set(ru.LN_STRIDED) == {(5, 7, 256), (5, 7, 768)}
    assert set(ru.LN_SELECTIONS) == {"dx", "dxsum", "dgb", "all"}
    # more rows than one pass of the 512-workgroup grid takes (8 a workgroup): some wave takes a second row
    assert all(rows > 4096 for rows, _ in ru.LN_MANY)
    by_d, by_nl = {}, {}
    for D, n, L in ru.EMBED_CASES:
        by_d.setdefault(D, []).append(n)
        by_nl.setdefault((n, L), set()).add(D)
    assert set(by_d) == {256, 512, 768, 1024} and set(by_nl) == {(1, 2), (3, 50), (5, 64), (9, 17)}
    for D, ns in by_d.items():
        assert any(n < 4 for n in ns) and any(n > 4 and n % 4 for n in ns), (D, ns)
    assert all(len(ds) >= 2 for ds in by_nl.values())
    assert ru.ROW_N == (1, 4, 5, 257) and ru.ROW_D == (1, 63, 64, 65, 100, 512)
    assert ru.CLIP_D == (63, 64, 65, 100, 512) and ru.CLIP_T == (2, 5, 64) and ru.ELEM_N == (1, 255, 256, 257, 1000)
    assert ru.HSC_NORMS == (1e-3, 1e-2, 1.0, 30.0)
    for cases, heads in ((ru.hsc_cases_all(), 2), (ru.dsad_cases_all(), 2)):
        assert {(c[0], c[1]) for c in cases} >= {(n, d) for n in ru.ROW_N for d in ru.ROW_D}
        assert {c[2] for c in cases} == {0, 1} and any(c[3] == "edge" for c in cases)
    assert set(ru.dsvdd_cases_all()) == {(n, d) for n in ru.ROW_N for d in ru.ROW_D}
    assert {(c[0], c[1]) for c in ru.elem_cases_all()} >= {(h, n) for h in ("bce", "focal") for n in ru.ELEM_N}
    assert len(ru.clip_cases_all()) == len(ru.ROW_N) * len(ru.CLIP_D) * len(ru.CLIP_T) * 4


def test_edge_rows_are_what_they_claim():
    # HSC: every norm in both label classes, and an all-zero row in each
    c = ru.hsc_case(0, 100, 0, "edge")
    norms = np.sqrt((c["f"].astype(np.float64) ** 2).sum(1))
    for label in (0, 1):
        got = norms[c["y"] == label]
        assert np.allclose(got[:-1], ru.HSC_NORMS, rtol=1e-6) and got[-1] == 0.0
    # the anomalous all-zero row: loss -log(1e-9), gradient exactly zero and finite (the exact expectations of test_hsc_bce)
    z = np.flatnonzero((norms == 0) & (c["y"] == 1))[0]
    assert abs(float(c["ref"]["rows"][z]) - 20.7233) < 1e-3 and float(c["ref"]["grad"][z].abs().max()) == 0.0
    # DSAD: an anomalous all-zero row (loss 1 / 1e-9, gradient 0) and anomalous rows at |f|^2 ~ 1e-3
    for nominal in (0, 1):
        c = ru.dsad_case(0, 100, nominal, "edge")
        ss = (c["f"].astype(np.float64) ** 2).sum(1)
        anom = c["y"] != nominal
        z = np.flatnonzero((ss == 0) & anom)
        assert len(z) == 1 and float(c["ref"]["rows"][z[0]]) == 1.0 / 1e-9 and float(c["ref"]["grad"][z[0]].abs().max()) == 0.0
        assert float(c["got32"]["rows"][z[0]]) == float(np.float32(1.0) / np.float32(1e-9))
        assert ((ss[anom] > 3e-4) & (ss[anom] < 3e-3)).sum() >= 2
        assert torch.isfinite(c["got32"]["grad"]).all()


def test_clip_cases_hold_a_live_tie_and_a_foreign_label():
    for n, d, T, loo, nominal in ru.clip_cases_all():
        c = ru.clip_case(n, d, T, loo, nominal)
        if n >= 4:
            assert c["y"][3] == 7 and float(c["ref"]["grad"][3].abs().max()) == 0.0
        if T >= 3:
            logits = oobj.clip_logits(torch.from_numpy(c["f"]).double(), torch.from_numpy(c["t"]).double())[0, :T - 1]
            assert c["y"][0] == nominal and logits[1] == logits[2] == logits.max()
        assert float(np.sqrt((c["f"].astype(np.float64) ** 2).sum(1)).min()) > 0.5 * np.sqrt(d) * 0.5
