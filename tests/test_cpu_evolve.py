"""CPU tier: the evolutionary OE-sample search (eoe_amd.evolve) on its numpy path -- the operators against the ids the
reference's own operators chose (fixture g21_evolve), the integer distances against the reference's fp32 ones, the driver with an
injected fitness, the two named error cases, the argument checks of the new entry points (all made before anything is launched),
and `oe_limit_samples` / `set_oe_subset` on the host side."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import evolve_util as eu


@pytest.fixture(scope="module")
def pool():
    from eoe_amd.evolve import OEPool
    return OEPool(torch.from_numpy(eu.pool_u8()))


def _run_case(pool, name, seed):
    from eoe_amd.evolve import mate_individuals, mutate_individual
    kind, inds, indp = eu.CASES[name]
    inds = [list(i) for i in inds]
    np.random.seed(int(seed))
    if kind == "mutate":
        assert mutate_individual(inds[0], pool, eu.POOLSIZE, indp, eu.ONEOFKBEST) == (inds[0],)
    else:
        assert mate_individuals(inds[0], inds[1], pool, eu.POOLSIZE, indp, eu.ONEOFKBEST) == (inds[0], inds[1])
    return inds


@pytest.mark.parametrize("name", list(eu.CASES))
def test_operators_choose_the_reference_ids(golden, pool, name):
    g = golden("g21_evolve")
    got = _run_case(pool, name, g[f"{name}/seed"])
    assert got == g[f"{name}/out"].tolist()
    assert got != [list(i) for i in eu.CASES[name][1]]                       # the case does change its individuals


def test_selection_chooses_the_reference_survivors(golden):
    from eoe_amd.evolve import Individual, select_individual
    g = golden("g21_evolve")
    pop = []
    for i, f in enumerate(eu.SELECT_FITS):
        pop.append(Individual([i]))
        pop[-1].fitness.values = (f,)
    np.random.seed(int(g["select/seed"]))
    chosen = select_individual(pop, len(pop), eu.SELECT_TOURNSIZE)
    assert [c[0] for c in chosen] == g["select/chosen"].tolist()


def _case_vectors(g, pool, name):
    """(integer distances, device-independent order, reference fp32 distances, candidate ids) of every vector the reference sorted"""
    kind, inds, _ = eu.CASES[name]
    for (n, li), ref in zip(g[f"{name}/owners"].tolist(), g[f"{name}/dist"]):
        cands = g[f"{name}/cands"][li].tolist()
        if kind == "mutate":
            dist, order = pool.distances(inds[0], cands)
            yield dist[n], order[n], ref, cands
        else:
            val = pool.distances([inds[0][0], inds[1][0]], cands)[0].sum(axis=0)
            yield val, np.argsort(val, kind="stable"), ref, cands


def test_integer_distances_match_the_reference(golden, pool):
    g = golden("g21_evolve")
    seen = 0
    for name in eu.CASES:
        for val, order, ref, cands in _case_vectors(g, pool, name):
            assert val.dtype == np.int64
            ref = ref.astype(np.float64)
            assert np.all(np.abs(val / 255.0 ** 2 - ref) <= 1e-4 * np.abs(ref))
            # the maker asserted gaps >= 0.05 between distinct ids, so the order by id is defined: the exact one equals fp32's
            assert [cands[i] for i in order] == [cands[i] for i in np.argsort(ref, kind="stable")]
            assert np.all(np.diff(val[order]) >= 0)
            seen += 1
    assert seen >= 5
    # the fixture's special candidates: the parent itself (0) and its near-duplicate (64 bytes off by 16: 0.25 < 100)
    dist, order = pool.distances([eu.PARENT], [eu.NEAR_DUP, eu.PARENT, 11, eu.PARENT])
    assert dist[0, 1] == 0 == dist[0, 3] and dist[0, 0] == 64 * 16 * 16 and order[0].tolist()[:3] == [1, 3, 0]
    from eoe_amd.evolve import SELF_THRESHOLD
    assert SELF_THRESHOLD == 6502500 and dist[0, 0] < SELF_THRESHOLD < dist[0, 2]


def test_pool_maps_ids_through_valid_indices():
    from eoe_amd.evolve import OEPool, init_individual, replace_individuals_randomly
    u8 = torch.from_numpy(eu.pool_u8())
    full, part = OEPool(u8), OEPool(u8, valid_indices=[40, 3, 7, 11])
    assert len(full) == eu.POOL_N and len(part) == 4 and part.rows([1, 2, 1]).tolist() == [3, 7, 3]
    assert np.array_equal(part.distances([1], [2, 0, 1])[0], full.distances([3], [7, 40, 3])[0])
    with pytest.raises(IndexError):
        part.rows([4])
    with pytest.raises(ValueError):
        OEPool(u8, valid_indices=[60])
    with pytest.raises(ValueError):
        part.distances([], [1])
    np.random.seed(3)
    want = [int(np.random.randint(0, 4)) for _ in range(3)]
    np.random.seed(3)
    assert [init_individual(part) for _ in range(2)] == want[:2]
    assert replace_individuals_randomly([9], part) == want[2:]


def test_the_reference_crash_cases_are_named_errors():
    from eoe_amd.evolve import OEPool, mate_individuals, mutate_individual
    same = OEPool(torch.full((5, 32, 32, 3), 9, dtype=torch.uint8))
    np.random.seed(0)
    with pytest.raises(ValueError, match="beyond the self-exclusion threshold"):
        mutate_individual([0], same, 10, 1.0, 3)
    with pytest.raises(ValueError, match="beyond the self-exclusion threshold"):
        mate_individuals([0], [1], same, 10, 1.0, 3)
    far = torch.zeros((4, 32, 32, 3), dtype=torch.uint8)
    far[1:] = 255
    np.random.seed(0)
    assert [np.random.randint(0, 4) for _ in range(2)] == [0, 3]             # this seed draws the parent itself and one far image
    np.random.seed(0)
    with pytest.raises(ValueError, match="only 1 of the 2 candidates lie beyond the self-exclusion threshold, fewer than oneofkbest = 3"):
        mutate_individual([0], OEPool(far), 2, 1.0, 3)


def _fitness(calls):
    def f(ind):
        calls.append(list(ind))
        return ((sum(ind) * 37) % 101) / 101.0
    return f


def _evolution(pool, calls, **kw):
    from eoe_amd.evolve import run_evolution
    np.random.seed(11)
    random.seed(11)
    args = dict(oesize=2, generation_pool=6, mutation_pool=30, mutation_indp=0.7, mutation_oneofkbest=3, mutation_chance=0.6,
                mate_chance=0.5, generations=4, select_toursize=3)
    args.update(kw)
    return run_evolution(None, pool, [0], 1, fitness_fn=_fitness(calls), **args)


def test_driver_is_deterministic_and_evaluates_only_unset_individuals(pool):
    calls1, calls2 = [], []
    h1, h2 = _evolution(pool, calls1), _evolution(pool, calls2)
    assert h1 == h2 and calls1 == calls2
    for k in ("pop", "fit", "mean_fit", "std_fit", "max_fit", "min_fit"):
        assert len(h1[k]) == 4, k
    assert set(h1["setup"]) == {"oesize", "geneation_pool", "mutation_pool", "mutation_indp", "mutation_oneofkbest", "mutation_chance",
                                "mate_chance", "generations", "oeds", "select_toursize"}
    assert all(len(p) == 6 and all(len(ind) == 2 for ind in p) for p in h1["pop"])
    for fits, mean, lo, hi in zip(h1["fit"], h1["mean_fit"], h1["min_fit"], h1["max_fit"]):
        assert mean == float(np.mean(fits)) and lo == min(fits) and hi == max(fits)
    # generation 0 trains everyone; later ones only what mating or mutation touched: fewer than the population, more than none
    assert calls1[:6] == h1["pop"][0] and 6 < len(calls1) < 4 * 6
    # every fitness in the history is the injected function of its ids
    for p, fits in zip(h1["pop"], h1["fit"]):
        assert fits == [((sum(ind) * 37) % 101) / 101.0 for ind in p]


def test_evaluate_counts_and_genealogy(pool, tmp_path):
    from eoe_amd.evolve import Genealogy, Individual, Toolbox, evaluate, run_evolution
    from eoe_amd.training.ad_trainer import JsonLogger
    import json
    calls, tree = [], Genealogy()
    off = [Individual([i]) for i in range(4)]
    for ind in off:
        tree.add(ind)
    off[1].fitness.values, off[3].fitness.values = (0.25,), (0.5,)
    history = {k: [] for k in ("pop", "fit", "mean_fit", "std_fit", "max_fit", "min_fit")}
    pop = []
    evaluate(off, pop, 0, Toolbox(evaluate=_fitness(calls)), history, tree)
    assert calls == [[0], [2]] and pop == off and history["fit"] == [[0.0, 0.25, 74 / 101.0, 0.5]]
    assert [n["fitness"] for n in tree.to_json()] == [0.0, None, 74 / 101.0, None]

    class T:                                   # what run_evolution needs of a trainer when the fitness is injected: its logger
        logger = JsonLogger(str(tmp_path))
        oe_dsstr = "pool60"

    np.random.seed(2)
    random.seed(2)
    calls = []
    h = run_evolution(T(), pool, [0], 1, fitness_fn=_fitness(calls), generation_pool=4, mutation_pool=20, generations=3)
    with open(tmp_path / "evolve_results.json") as f:
        assert json.load(f) == h and h["setup"]["oeds"] == "pool60"
    with open(tmp_path / "evolution.json") as f:
        nodes = json.load(f)
    assert [n["id"] for n in nodes] == list(range(len(nodes))) and set(nodes[0]) == {"id", "generation", "ids", "fitness", "parents"}
    assert all(n["parents"] == [] and n["generation"] == 0 for n in nodes[:4]) and len(nodes) > 4
    assert all(n["parents"] and all(p < n["id"] for p in n["parents"]) for n in nodes[4:])
    assert len(calls) == sum(n["fitness"] is not None for n in nodes)          # one training per evaluated node, none twice
    # the random baseline: one generation of random subsets
    h = run_evolution(None, pool, [0], 1, fitness_fn=_fitness([]), generation_pool=5, oesize=3, random_pick=True)
    assert len(h["fit"]) == 1 and len(h["pop"][0]) == 5 and h["setup"] == {"oesize": 3}


def test_minimize_fitness_reverses_the_selection(pool):
    from eoe_amd.evolve import evolve_setup, select_individual
    for maxfit, want in ((True, 2), (False, 3)):
        pop, gen, toolbox, history, tree = evolve_setup(1, 8, 10, 1.0, 3, 0.5, 0.2, 2, 8, pool, None, maxfit=maxfit)
        for i, (ind, f) in enumerate(zip(pop, eu.SELECT_FITS)):
            ind[0] = i
            ind.fitness.values = (f,)
        np.random.seed(0)
        chosen = toolbox.select(pop, 5)                     # a tournament of the whole population: its best, every time
        assert [c[0] for c in chosen] == [want] * 5
    np.random.seed(4)
    a = select_individual(pop, 8, 3)
    np.random.seed(4)
    aspirants = [[pop[i] for i in np.random.choice(8, 3, False)] for _ in range(8)]
    assert [c[0] for c in a] == [min(asp, key=lambda x: x.fitness.values[0])[0] for asp in aspirants]
    calls = []
    h_max, h_min = _evolution(pool, calls, generations=6), _evolution(pool, calls, generations=6, minimize_fitness=True)
    assert h_max["pop"][0] == h_min["pop"][0] and h_max["pop"][1] != h_min["pop"][1]


def test_driver_refuses_more_than_one_class():
    from eoe_amd.evolve import run_evolution

    class T:
        ds = None
    for classes in ([0, 1], [], None):
        with pytest.raises(NotImplementedError, match="multiple classes"):
            run_evolution(T(), None, classes)


# ---------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_check_their_arguments_before_launching():
    from eoe_amd import _lib
    lib = _lib.lib
    assert _lib.ABI_VERSION == 5 and lib.eoe_abi_version() == 5               # additive: the ABI version does not move
    assert {"eoe_pool_sqdist_workspace", "eoe_pool_sqdist_u8", "eoe_pool_rank"} <= set(_lib.header_symbols())
    need = C.c_size_t(0)
    assert lib.eoe_pool_sqdist_workspace(3072, 1, 100, C.byref(need)) == 0 and need.value >= 101 * 4 + 100 * 3 * 4
    assert lib.eoe_pool_sqdist_workspace(189, 5, 7, C.byref(need)) == 0 and 48 <= need.value <= 256      # one chunk: the indices alone
    for D, K, P in ((0, 1, 1), (3072, 0, 1), (3072, 1, 0), (3072, 1025, 1), ((1 << 26) + 1, 1, 1)):
        assert lib.eoe_pool_sqdist_workspace(D, K, P, C.byref(need)) == 1, (D, K, P)
    # fake, never dereferenced device pointers: every call below must return before anything is read or launched
    SET, OUT, WS = 0x1000, 0x2000, 0x3000
    q, c = np.array([0], np.int32), np.array([1, 2, 59], np.int32)

    def sqdist(q, c, n_set=60, K=None, P=None, ws_bytes=1 << 20):
        return lib.eoe_pool_sqdist_u8(SET, n_set, 3072, q.ctypes.data, len(q) if K is None else K, c.ctypes.data,
                                      len(c) if P is None else P, OUT, WS, ws_bytes, None)

    for bad_c in ([1, 60, 2], [1, -1, 2]):
        assert sqdist(q, np.array(bad_c, np.int32)) == 1
        assert b"candidate 1" in lib.eoe_last_error() and b"outside the set of 60 rows" in lib.eoe_last_error()
    assert sqdist(np.array([60], np.int32), c) == 1 and b"query 0" in lib.eoe_last_error()
    assert sqdist(q, c, K=0) == 1 and b"K (queries)" in lib.eoe_last_error()
    assert sqdist(q, c, P=0) == 1 and b"P (candidates)" in lib.eoe_last_error()
    assert sqdist(q, c, ws_bytes=8) == 1 and b"workspace" in lib.eoe_last_error()
    assert lib.eoe_pool_sqdist_u8(None, 60, 3072, q.ctypes.data, 1, c.ctypes.data, 3, OUT, WS, 1 << 20, None) == 1
    assert lib.eoe_pool_rank(OUT, 1, 1025, WS, None) == 3 and b"at most 1024" in lib.eoe_last_error()     # EOE_ERR_UNSUPPORTED
    assert lib.eoe_pool_rank(OUT, 1, 0, WS, None) == 1 and lib.eoe_pool_rank(OUT, 0, 5, WS, None) == 1
    assert lib.eoe_pool_rank(None, 1, 5, WS, None) == 1


# ------------------------------------------------------------------------------------------------- trainer / source wiring
class _Source:
    """a step-batch source that records what `set_oe_subset` is asked"""
    nominal_label, normalize = 0, None

    def __init__(self, n_oe=10):
        self.oe, self.asked = torch.zeros((n_oe, 4, 4, 3), dtype=torch.uint8), []

    def loaders(self, batch_size=None, **kw):
        return [], []

    def set_oe_subset(self, rows):
        self.asked.append(rows)


def _trainer(**kw):
    from eoe_amd.training import HSCTrainer
    return HSCTrainer(torch.nn.Linear(2, 2), device="cpu", **kw)


def test_default_oe_limit_leaves_the_source_alone():
    from eoe_amd.data import ListSource
    src = _Source()
    for kw in ({}, {"oe_limit_samples": np.inf}, {"oe_limit_samples": float("inf")}):
        tr = _trainer(dataset=src, **kw)
        assert tr._dataset(0, 0) is src and src.asked == []
    plain = ListSource([])                                   # a source without set_oe_subset keeps working under the default ...
    assert _trainer(dataset=plain)._dataset(0, 0) is plain
    with pytest.raises(NotImplementedError, match="set_oe_subset"):      # ... and a limit it cannot honour is no longer dropped silently
        _trainer(dataset=plain, oe_limit_samples=3)._dataset(0, 0)


def test_oe_limit_samples_reaches_the_source():
    src = _Source(10)
    assert _trainer(dataset=src, oe_limit_samples=[4, 2, 4])._dataset(0, 0) is src and src.asked == [[4, 2, 4]]
    np.random.seed(5)
    want = sorted(int(i) for i in np.random.choice(10, 3, False))
    np.random.seed(5)
    _trainer(dataset=src, oe_limit_samples=3)._dataset(0, 0)
    assert src.asked[-1] == want and len(want) == 3
    _trainer(dataset=src, oe_limit_samples=50)._dataset(0, 0)              # more than there is: all rows, once each
    assert src.asked[-1] == list(range(10))
    made = []
    tr = _trainer(dataset=lambda c, seed: made.append(_Source(6)) or made[-1], oe_limit_samples=[5])
    assert tr._dataset(0, 0) is made[0] and made[0].asked == [[5]]          # a callable's source is restricted as well
    with pytest.raises(ValueError):
        _trainer(dataset=src, oe_limit_samples=0)._dataset(0, 0)


def test_set_oe_subset_validates_and_restores():
    from eoe_amd.data import LabelledImageSet, ResidentImageSource
    u8 = torch.zeros((6, 8, 8, 3), dtype=torch.uint8)
    src = ResidentImageSource(u8, u8, u8, torch.tensor([0, 1, 0, 1, 0, 1]), crop=8, device="cpu")
    assert src.oe_subset is None
    src.set_oe_subset([5, 0, 5])
    assert src.oe_subset.tolist() == [5, 0, 5] and src.oe_subset.dtype == torch.int64
    src.set_oe_subset(None)
    assert src.oe_subset is None
    for bad in ([6], [-1], []):
        with pytest.raises((IndexError, ValueError)):
            src.set_oe_subset(bad)
    assert src.oe_subset is None
    lab = torch.tensor([0, 1, 0, 1, 0, 1])
    lset = LabelledImageSet(u8, lab, u8, lab, u8, ["a", "b"], 8, device="cpu")
    assert lset.source([0]).oe_subset is None and lset.source([0], oe_subset=[2, 3]).oe_subset.tolist() == [2, 3]
