"""Generates tests/golden/g21_evolve.npz by running the REFERENCE's own evolve operators (`evolve/__init__.py`:
`mutate_individual`, `mate_individuals`, `select_individual`) on a list-like OE dataset without transforms.  Run by hand where the
reference is available; the tests only read the .npz.

    python tests/golden/make_golden_evolve.py <the reference's src/eoe directory>

The reference module is loaded by file path, nothing re-typed; what it imports and this experiment does not need is stubbed in
`sys.modules` (`deap.base`, `deap.tools.selection` with `attrgetter = operator.attrgetter`, `eoe.evolve.tree`,
`eoe.training.ad_trainer`, `eoe.utils.logger`).  What it computes is observed from outside: `torch.Tensor.sort` is wrapped to
keep every distance vector the operators sort, `np.random.randint` to keep the candidate ids they draw.

Inputs (tests/evolve_util.py): 60 images of 32 x 32 x 3, image 7 a near-duplicate of image 3 (distance 0.25 < 100).  Per case
the seed is the first one at which the case shows what it is for (the parent AND its near-duplicate among the candidates, and
the individual changed, and the order of every sorted vector is defined as below); the record holds it.

Asserted here, so that the order the tests compare is defined: for every sorted distance vector, the reference's fp32 distances
of DISTINCT candidate ids differ by at least 0.05, far above fp32 summation error at these magnitudes (<= 3 000, 3 072 terms);
repeated ids tie exactly and select the same id whichever tie position is drawn.
"""
import importlib.util
import operator
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
import evolve_util as eu   # noqa: E402

MIN_GAP = 0.05


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    return m


def load_reference(ref: str):
    blank = lambda n: type(n, (), {})      # noqa: E731
    _stub("deap")
    _stub("deap.base", Toolbox=blank("Toolbox"))
    _stub("deap.tools")
    _stub("deap.tools.selection", attrgetter=operator.attrgetter)
    _stub("eoe")
    _stub("eoe.training")
    _stub("eoe.utils")
    _stub("eoe.evolve.tree", Node=blank("Node"), Tree=blank("Tree"), EvolNode=blank("EvolNode"), Individual=blank("Individual"))
    _stub("eoe.training.ad_trainer", ADTrainer=blank("ADTrainer"))
    _stub("eoe.utils.logger", Logger=blank("Logger"))
    spec = importlib.util.spec_from_file_location("eoe.evolve", os.path.join(ref, "evolve", "__init__.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["eoe.evolve"] = m
    spec.loader.exec_module(m)
    return m


class FakeOE:
    """what the operators need of the OE `Subset`: len, `[id] -> (image, label, index)`, `.indices`; ToTensor'd, no transform"""

    def __init__(self, u8_nhwc: np.ndarray):
        self.x = torch.from_numpy(u8_nhwc).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
        self.indices = list(range(len(self.x)))

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[int(i)], 1, int(i)


class Watch:
    """records the vectors passed to Tensor.sort and the results of np.random.randint while active"""

    def __enter__(self):
        self.sorted, self.drawn = [], []
        self._sort, self._randint = torch.Tensor.sort, np.random.randint
        watch = self

        def sort(t, *a, **k):
            watch.sorted.append(t.detach().clone())
            return watch._sort(t, *a, **k)

        def randint(*a, **k):
            r = watch._randint(*a, **k)
            watch.drawn.append(int(r))
            return r

        torch.Tensor.sort, np.random.randint = sort, randint
        return self

    def __exit__(self, *exc):
        torch.Tensor.sort, np.random.randint = self._sort, self._randint


def min_gap(dist: torch.Tensor, cands) -> float:
    """the least difference between the distances of distinct candidate ids in one sorted vector"""
    by_id = {}
    for d, c in zip(dist.tolist(), cands):
        assert by_id.setdefault(c, d) == d                   # a repeated id ties exactly
    return float(np.diff(np.sort(np.array(list(by_id.values())))).min())


def owners_of(ds, kind, inds, cands, sorted_vectors):
    """which (image of the individual, candidate list) every sorted vector belongs to: the reference's own expression, compared
    exactly"""
    owners = []
    for d in sorted_vectors:
        found = None
        for li, c in enumerate(cands):
            new_samples = torch.stack([ds[i][0] for i in c])
            if kind == "mutate":
                for n, i in enumerate(inds[0]):
                    if torch.equal((ds[i][0].unsqueeze(0) - new_samples).pow(2).flatten(1).sum(1), d):
                        found = (n, li)
            else:
                double = torch.stack([ds[inds[0][0]][0], ds[inds[1][0]][0]])
                if torch.equal((double.unsqueeze(1) - new_samples).pow(2).flatten(2).sum(-1).sum(0), d):
                    found = (0, li)
        assert found is not None
        owners.append(found)
    return owners


def run_case(ref, ds, kind, inds, indp, seed):
    np.random.seed(seed)
    inds = [list(i) for i in inds]
    with Watch() as w:
        if kind == "mutate":
            ref.mutate_individual(inds[0], ds, eu.POOLSIZE, indp, eu.ONEOFKBEST)
        else:
            ref.mate_individuals(inds[0], inds[1], ds, eu.POOLSIZE, indp, eu.ONEOFKBEST)
    return inds, w


def main():
    ref = load_reference(sys.argv[1])
    u8 = eu.pool_u8()
    ds = FakeOE(u8)
    out = {}
    for name, (kind, inds, indp) in eu.CASES.items():
        single = len(inds[0]) == 1
        lists = 0 if (kind == "mate" and not single) else (1 if kind == "mutate" else 2)
        for seed in range(1000):
            got, w = run_case(ref, ds, kind, inds, indp, seed)
            cands = [w.drawn[i * eu.POOLSIZE:(i + 1) * eu.POOLSIZE] for i in range(lists)]
            if got == [list(i) for i in inds]:
                continue
            if single and not all(eu.PARENT in c and eu.NEAR_DUP in c for c in cands):
                continue
            if name == "mutate4" and len(w.sorted) < 2:       # at least two of the four images replaced
                continue
            owners = owners_of(ds, kind, inds, cands, w.sorted)
            if any(min_gap(d, cands[li]) < MIN_GAP for d, (_, li) in zip(w.sorted, owners)):
                continue                     # two distinct candidates closer than fp32 can be trusted to order: not a defined case
            break
        else:
            raise AssertionError(name)
        for d, (_, li) in zip(w.sorted, owners):
            assert min_gap(d, cands[li]) >= MIN_GAP
        assert len(w.sorted) > 0 or lists == 0
        if name == "mutate1":                    # the near-duplicate sits under the threshold, right after the parent itself
            d, c = w.sorted[0], cands[0]
            assert d[c.index(eu.PARENT)].item() == 0.0 and 0.0 < d[c.index(eu.NEAR_DUP)].item() < 100.0
        out[f"{name}/seed"] = np.int64(seed)
        out[f"{name}/out"] = np.asarray(got, np.int64)
        out[f"{name}/cands"] = np.asarray(cands, np.int64).reshape(lists, eu.POOLSIZE)
        out[f"{name}/owners"] = np.asarray(owners, np.int64).reshape(len(owners), 2)
        out[f"{name}/dist"] = torch.stack(w.sorted).numpy() if w.sorted else np.zeros((0, eu.POOLSIZE), np.float32)
        print(name, "seed", seed, inds, "->", got, "sorted vectors", len(w.sorted), owners)

    # ---- tournament selection: individuals [i] with fitness SELECT_FITS[i]
    class Ind(list):
        pass

    pop = []
    for i, f in enumerate(eu.SELECT_FITS):
        ind = Ind([i])
        ind.fitness = f
        pop.append(ind)
    seed = 5
    np.random.seed(seed)
    chosen = ref.select_individual(pop, len(pop), eu.SELECT_TOURNSIZE)
    out["select/seed"] = np.int64(seed)
    out["select/chosen"] = np.asarray([c[0] for c in chosen], np.int64)
    assert len(set(out["select/chosen"].tolist())) > 2
    print("select", out["select/chosen"])

    path = os.path.join(HERE, "g21_evolve.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
