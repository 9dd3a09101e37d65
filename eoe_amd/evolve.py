"""The evolutionary search for good outlier-exposure (OE) samples: `src/eoe/evolve/__init__.py` and the setup functions of
`src/eoe/main/__init__.py:320-482`, without DEAP.

An individual is a list of OE ids (positions in the pool's `valid_indices`, as in the reference, `evolve/__init__.py:42-52`); its
fitness is the mean test AUC of a short `trainer.run` with exactly those OE images.  A generation is select -> mate -> mutate ->
evaluate (`:252-357`).

The candidate search of mutation and mating runs on the device: the reference pulls `poolsize` (100) candidate images through
the host dataset one at a time and measures their squared distance to the parent on the host (`:100-157`), for every mutated or
mated individual; here the images already sit in HBM as uint8 and `OEPool.distances` is a gather, one distance kernel and one
rank kernel (`csrc/evolve.hip`), with one small copy back.

A pool of MIXED sizes (`RaggedImageSet`: the 224 x 224 tasks after `Resize(256)`, `main/evolve_oe_imagenet.py`,
`main/evolve_oe_custom.py`) is searched without resizing anything to a common shape: `OEPool(rs, crop=224)` or
`OEPool.from_source(src)` compares each image's `CenterCrop(crop)` window -- the stored-bytes analogue there, the window the test
split scores and `normalize=` fits over, zero-padded for an image smaller than the crop -- with `eoe_pool_sqdist_ragged_u8`, which
reads the windows straight out of the arena.  `run_evolution(trainer, OEPool.from_source(trainer.ds), ...)` runs such a search; the
default `pool=None` keeps refusing a ragged OE set, since it cannot know the window.

What differs from the reference, deliberately:
  * Distances are taken on the STORED images (after the source's one-time resize), as exact integers.  The reference's
    `oeds[id][0]` passes every image through the random train transform (jitter, crop, flip, noise) each time it is fetched, so
    its distances are stochastic and no bit parity is defined; on untransformed images the decisions are the same (golden test).
  * The self-exclusion rule `val > 100` in the [0, 1] pixel scale is `d > 100 * 255^2 = 6 502 500` on the integers, exactly.
  * The operators draw from `np.random` / `random` in the reference's order (pool ids first, then per OE image
    `np.random.rand() < indp`, then `np.random.randint(s, s + oneofkbest)`), so with equal distances the decisions are identical.
  * The reference's two crash cases (no candidate beyond the threshold: StopIteration; `s + oneofkbest` past the pool:
    IndexError) raise a ValueError that names the cause.
  * `evaluate` trains only the individuals whose fitness is unset (the reference's `ind in invalid_ind` compares id lists, so a
    valid twin of an invalid individual is trained again); `history['pop']` holds a copy of each generation's id lists (the
    reference appends the one population object it keeps overwriting).
  * The figures (`run_evolution(log_images=True)`; `evolve/__init__.py:209-240, 278-355`, `evolve/tree.py:262-340`) are composed on
    the device from (pool, ids) by `logger.logimg` -> `eoe_amd.imgrid.image_grid`: no image tensor is built on the host, where the
    reference fetches every image through the dataset (and its random train transform) again for each figure.  They show the
    STORED images (a ragged pool: the centre windows the distances are taken on).  The sorted `gen{g}` grid orders whole
    individuals by fitness (stable); the reference zips the fitness list with the flat image list, which pairs -- and keeps -- only
    the first `len(pop)` images once an individual holds more than one.  The "best / worst k" figures compose the chosen
    individuals' strips again from the pool (one launch pair for all k) rather than re-reading their PNG files; the second pass
    normalises the first pass's bytes, as the reference's does.  `mark`'s frame colours and the other stated differences of the
    pictures themselves: `eoe_amd/imgrid.py`.
  * Out of scope: `Tree.vis` (the graphviz genealogy plot), the `final-transformed` MSM figures, text drawn into pictures (row
    headers go to `<name>.headers.json`), `--ev-continue-run`, the CLI runners.
"""
import os
import random
from copy import deepcopy
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

SELF_THRESHOLD = 100 * 255 * 255          # the reference's `val > 100` (evolve/__init__.py:113,119,154) on integer distances
RANK_MAX_CANDIDATES = 1024                # eoe_pool_rank


# --------------------------------------------------------------------------------------------------------------- the pool
class OEPool:
    """the complete OE set the search draws from and `valid_indices`, the rows an id may name (`evolve/__init__.py:42-52`; default:
    all rows).  The set is uint8 images [n, H, W, C] (a GPU tensor: the kernels; a CPU tensor: numpy int64 with the same results),
    compared whole, or a `RaggedImageSet` with `crop=` (an int or (h, w)): images of mixed sizes have no common shape, so what is
    compared is each image's `CenterCrop(crop)` window, zero-padded where the image is smaller (`data.center_origins`)"""

    def __init__(self, oe_u8, valid_indices=None, crop=None):
        from .data import RaggedImageSet, center_origins
        self.crop = self._origins = None
        if isinstance(oe_u8, RaggedImageSet):
            if crop is None:
                raise NotImplementedError("the candidate search measures distances between OE images of ONE shape; a RaggedImageSet has "
                                          "none (pass crop=: the CenterCrop(crop) windows are compared, OEPool.from_source takes the "
                                          "source's; or Resize the pool to one (h, w) first: resize_u8 with a pair gives the tensor)")
            ch, cw = (int(crop), int(crop)) if isinstance(crop, (int, np.integer)) else (int(v) for v in crop)
            if ch < 1 or cw < 1:
                raise ValueError(f"OEPool: crop must be positive, not {crop}")
            self.images, self.crop = oe_u8, (ch, cw)
            n, self.features = len(oe_u8), ch * cw * oe_u8.channels
            self._origins = np.stack([center_origins(oe_u8.sizes[:, 0], ch), center_origins(oe_u8.sizes[:, 1], cw)], axis=1).astype(np.int32)
        else:
            if crop is not None:
                raise ValueError("OEPool: crop= selects the windows of a RaggedImageSet; a tensor set is compared whole")
            if oe_u8.dtype != torch.uint8 or oe_u8.dim() < 2:
                raise ValueError("OEPool needs a uint8 image set [n, ...]")
            self.images = oe_u8.contiguous()
            n, self.features = self.images.shape[0], int(np.prod(self.images.shape[1:]))
        self.valid_indices = np.arange(n, dtype=np.int64) if valid_indices is None else np.asarray(valid_indices, dtype=np.int64).reshape(-1)
        if len(self.valid_indices) == 0 or self.valid_indices.min() < 0 or self.valid_indices.max() >= n:
            raise ValueError(f"valid_indices must name rows of the set of {n} images, and at least one")
        self._workspace = None

    @classmethod
    def from_source(cls, src, valid_indices=None):
        """the pool of a source's resident OE set (`ResidentImageSource.oe`): a tensor set as it is, a ragged one with the source's
        crop -- the window its test split scores and `normalize=` fits over"""
        from .data import RaggedImageSet
        return cls(src.oe, valid_indices, crop=src.crop if isinstance(src.oe, RaggedImageSet) else None)

    def __len__(self) -> int:
        return len(self.valid_indices)

    def rows(self, ids) -> np.ndarray:
        """ids (positions in valid_indices) -> rows of the image set"""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if len(ids) and (ids.min() < 0 or ids.max() >= len(self)):
            raise IndexError(f"OE id outside the pool of {len(self)} samples")
        return self.valid_indices[ids]

    def distances(self, query_ids, cand_ids) -> Tuple[np.ndarray, np.ndarray]:
        """squared distances of every query image to every candidate image, on the stored bytes (a ragged set: on the centre
        windows): (int64 [K, P], int32 [K, P]) = (the distances, per query the stable ascending order of them as positions in
        `cand_ids`), both on the host"""
        q, c = self.rows(query_ids).astype(np.int32), self.rows(cand_ids).astype(np.int32)
        if len(q) < 1 or len(c) < 1:
            raise ValueError("distances need at least one query and one candidate")
        if self.images.is_cuda:
            return self._distances_device(q, c)
        if self.crop is not None:
            flat = self._windows_host(np.concatenate([q, c])).reshape(len(q) + len(c), -1).astype(np.int64)
            qi, ci = flat[:len(q)], flat[len(q):]
        else:
            flat = self.images.reshape(self.images.shape[0], -1).numpy()
            qi, ci = flat[q].astype(np.int64), flat[c].astype(np.int64)
        dist = np.stack([((ci - row) ** 2).sum(axis=1) for row in qi])
        return dist, np.argsort(dist, axis=1, kind="stable").astype(np.int32)

    def _windows_host(self, rows) -> np.ndarray:
        """uint8 [len(rows), crop_h, crop_w, C]: the centre windows of the listed images of a CPU ragged set, zero-padded"""
        (ch, cw), out = self.crop, np.zeros((len(rows), *self.crop, self.images.channels), dtype=np.uint8)
        for i, r in enumerate(rows):
            img, (top, left) = self.images[int(r)].numpy(), (int(v) for v in self._origins[r])
            H, W = img.shape[:2]
            y0, y1, x0, x1 = max(top, 0), min(top + ch, H), max(left, 0), min(left + cw, W)
            out[i, y0 - top:y1 - top, x0 - left:x1 - left] = img[y0:y1, x0:x1]
        return out

    def _distances_device(self, q: np.ndarray, c: np.ndarray):
        import ctypes
        from ._lib import check, lib
        K, P, dev = len(q), len(c), self.images.device
        need = ctypes.c_size_t(0)
        if self.crop is not None:
            check(lib.eoe_pool_sqdist_ragged_workspace(*self.crop, self.images.channels, K, P, ctypes.byref(need)),
                  "eoe_pool_sqdist_ragged_workspace")
        else:
            check(lib.eoe_pool_sqdist_workspace(self.features, K, P, ctypes.byref(need)), "eoe_pool_sqdist_workspace")
        if self._workspace is None or self._workspace.numel() < need.value:
            self._workspace = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
        # distances and order in ONE buffer (K * P int64, then K * P int32), so that both come back in one copy
        out = torch.empty(K * P * 12, dtype=torch.uint8, device=dev)
        dist, order = out[:K * P * 8].view(torch.int64), out[K * P * 8:].view(torch.int32)
        q, c = np.ascontiguousarray(q), np.ascontiguousarray(c)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            if self.crop is not None:
                # (row, top, left) of the queries, then of the candidates, in ONE array: the entry point uploads it in one copy
                rows, win = np.concatenate([q, c]), np.empty((K + P, 3), dtype=np.int32)
                win[:, 0], win[:, 1:] = rows, self._origins[rows]
                rs = self.images
                check(lib.eoe_pool_sqdist_ragged_u8(rs.arena.data_ptr(), rs.arena.numel(), rs.offsets.data_ptr(), rs.sizes_dev.data_ptr(),
                                                    len(rs), rs.channels, *self.crop, win.ctypes.data, K, win[K:].ctypes.data, P,
                                                    dist.data_ptr(), self._workspace.data_ptr(), self._workspace.numel(), stream),
                      "eoe_pool_sqdist_ragged_u8")
            else:
                check(lib.eoe_pool_sqdist_u8(self.images.data_ptr(), self.images.shape[0], self.features, q.ctypes.data, K, c.ctypes.data, P,
                                             dist.data_ptr(), self._workspace.data_ptr(), self._workspace.numel(), stream), "eoe_pool_sqdist_u8")
            check(lib.eoe_pool_rank(dist.data_ptr(), K, P, order.data_ptr(), stream), "eoe_pool_rank")
            host = out.cpu().numpy()             # synchronises: the index arrays q, c (win) were alive for the whole call
        return host[:K * P * 8].view(np.int64).reshape(K, P).copy(), host[K * P * 8:].view(np.int32).reshape(K, P).copy()


# ------------------------------------------------------------------------------------------------------------- individuals
class Fitness:
    """one weighted objective, as DEAP's `base.Fitness` with `weights=(1.0,)` (maximise) or `(-1.0,)` (minimise): comparisons
    go by weight * value, `valid` is False until a value is set"""

    def __init__(self, weight: float = 1.0):
        self.weight, self.values = float(weight), ()

    @property
    def valid(self) -> bool:
        return len(self.values) > 0

    @property
    def wvalues(self) -> tuple:
        return tuple(self.weight * v for v in self.values)

    def invalidate(self):
        self.values = ()

    def __gt__(self, other):
        return self.wvalues > other.wvalues

    def __lt__(self, other):
        return self.wvalues < other.wvalues

    def __ge__(self, other):
        return self.wvalues >= other.wvalues

    def __le__(self, other):
        return self.wvalues <= other.wvalues

    def __eq__(self, other):
        return self.wvalues == other.wvalues

    __hash__ = None


class Individual(list):
    """a list of OE ids with a fitness that may be unset, and the id of its node in the genealogy"""

    def __init__(self, ids=(), weight: float = 1.0):
        super().__init__(ids)
        self.fitness = Fitness(weight)
        self.node = None


class Genealogy:
    """who descends from whom: one node per created individual (id, generation, ids, fitness, parent ids).  A survivor of the
    selection is a clone that keeps pointing at its node; mating and mutation make new nodes"""

    def __init__(self):
        self.nodes = []

    def add(self, ind: Individual, parents: Sequence[int] = ()) -> int:
        self.nodes.append({"id": len(self.nodes), "generation": None, "ids": [int(i) for i in ind], "fitness": None,
                           "parents": sorted(set(int(p) for p in parents))})
        ind.node = len(self.nodes) - 1
        return ind.node

    def evaluated(self, ind: Individual, gen: int, fitness: float, file: str = None):
        """`file`: the path of the individual's picture (`node.content.file`, `evolve/__init__.py:219`); the key exists only on
        nodes whose picture was logged"""
        self.nodes[ind.node].update(generation=int(gen), fitness=float(fitness), ids=[int(i) for i in ind])
        if file is not None:
            self.nodes[ind.node]["file"] = file

    def to_json(self) -> list:
        return deepcopy(self.nodes)

    def scores_best(self, k: int = 20, reverse: bool = False, return_nodes: bool = False):
        """the fitness values of the k best evaluated individuals, ascending (`reverse`: of the k worst), as `tree.py:262-281`:
        nodes with a fitness, sorted by id list (stable) with repeats of an id list dropped (the first one is kept), then sorted by
        fitness (stable), then the last k (`reverse`: the first k).  `return_nodes`: (values, nodes).  Nodes are visited in the
        order of their creation where the reference walks its tree breadth-first; the two differ only in which of several nodes
        with EQUAL id lists, or in which order nodes of EQUAL fitness, are kept."""
        nodes = sorted((n for n in self.nodes if n["fitness"] is not None), key=lambda n: n["ids"])
        nodes = [n for i, n in enumerate(nodes) if i == 0 or n["ids"] != nodes[i - 1]["ids"]]
        nodes = sorted(nodes, key=lambda n: n["fitness"])
        nodes = (nodes[:k] if reverse else nodes[-k:]) if k > 0 else []
        fits = [n["fitness"] for n in nodes]
        return (fits, nodes) if return_nodes else fits

    def imsave_best(self, logger, pool: "OEPool", name: str, k: int = 20, reverse: bool = False, print_fitness: bool = False):
        """`tree.py:283-320`: one figure of the k best (`reverse`: worst) individuals.  Each individual's strip -- the picture of its
        `individuals/...` file, `nrow=16` -- is composed on the device, all k strips by ONE launch pair into one buffer; the strips
        are then composed again as uint8 cells with `maxres=1024`: side by side (`nrow=k`), or one per row with the fitness values as
        `rowheaders` (`print_fitness`).  The reference re-reads the PNG files and normalises a second time; here the second pass
        takes the first pass's bytes.  Returns the picture (None when nothing was evaluated)."""
        from .imgrid import image_grids
        fits, nodes = self.scores_best(k, reverse, return_nodes=True)
        if not nodes:
            return None
        if len({len(n["ids"]) for n in nodes}) != 1:
            raise ValueError("imsave_best: the individuals differ in their number of OE images; their strips have no common shape")
        strips = image_grids(pool, [n["ids"] for n in nodes], nrow=16)
        if print_fitness:
            return logger.logimg(name, strips, nrow=1, rowheaders=[f"{f * 100:06.3f}" for f in fits], maxres=1024)
        return logger.logimg(name, strips, nrow=k, maxres=1024)

    def imsave_collection_best(self, logger, pool: "OEPool", k: int = 20):
        """`tree.py:322-340` without the MSM figures: `final/best_raw`, `final/best`, `final/worst_raw`, `final/worst`"""
        self.imsave_best(logger, pool, os.path.join("final", "best_raw"), k=k)
        self.imsave_best(logger, pool, os.path.join("final", "best"), k=k, print_fitness=True)
        self.imsave_best(logger, pool, os.path.join("final", "worst_raw"), k=k, reverse=True)
        self.imsave_best(logger, pool, os.path.join("final", "worst"), k=k, reverse=True, print_fitness=True)


# --------------------------------------------------------------------------------------------------------------- operators
def init_individual(pool: OEPool) -> int:
    """a random OE id (`evolve/__init__.py:42-52`)"""
    return int(np.random.randint(0, len(pool.valid_indices)))


def _pick(val: np.ndarray, order: np.ndarray, oneofkbest: int, what: str) -> int:
    """the reference's choice among sorted candidates (`:153-155`): s = the first sorted position beyond the self-exclusion
    threshold, then one of the `oneofkbest` positions from s on; returns the chosen position in the candidate list"""
    beyond = np.nonzero(val[order] > SELF_THRESHOLD)[0]
    if len(beyond) == 0:
        raise ValueError(f"{what}: none of the {len(val)} candidates lies beyond the self-exclusion threshold (squared distance "
                         f"> 100 in the [0, 1] scale); the reference stops with StopIteration here")
    s = int(beyond[0])
    if s + oneofkbest > len(val):
        raise ValueError(f"{what}: only {len(val) - s} of the {len(val)} candidates lie beyond the self-exclusion threshold, fewer than "
                         f"oneofkbest = {oneofkbest}; the reference may index past the pool here")
    c = int(np.random.randint(s, s + oneofkbest))
    return int(order[c])


def mutate_individual(ind, pool: OEPool, poolsize: int, indp: float, oneofkbest: int) -> tuple:
    """`evolve/__init__.py:131-157`: a random candidate list; each OE image is replaced with probability `indp` by one of the
    `oneofkbest` candidates closest to it (beyond the self-exclusion threshold).  In place; returns (ind,)"""
    new_ids = [int(np.random.randint(0, len(pool))) for _ in range(poolsize)]
    dist = order = None
    if len(ind) > 0 and poolsize > 0:
        dist, order = pool.distances(list(ind), new_ids)       # all of the individual's images against the pool in one call
    for n in range(len(ind)):
        if np.random.rand() < indp:
            if dist is None:
                raise ValueError("mutate: the candidate pool is empty (poolsize = 0)")
            ind[n] = new_ids[_pick(dist[n], order[n], oneofkbest, "mutate")]
    return ind,


def mate_individuals(ind1, ind2, pool: OEPool, poolsize: int, indp: float, oneofkbest: int) -> tuple:
    """`evolve/__init__.py:81-128`.  Several OE images per individual: swap positions with probability `indp`.  One image each:
    two candidate lists; each parent's image is replaced (with probability `indp`) by one of the `oneofkbest` candidates of its
    list with the least SUMMED distance to both parents' images, an image "in between".  `match_samples` pairs the images of
    the two parents; it is only reached with one image per parent, where it pairs the two.  In place; returns (ind1, ind2)"""
    if len(ind1) == 1:
        pair = [ind1[0], ind2[0]]
        new_ids1 = [int(np.random.randint(0, len(pool))) for _ in range(poolsize)]
        new_ids2 = [int(np.random.randint(0, len(pool))) for _ in range(poolsize)]
        for ind, new_ids in ((ind1, new_ids1), (ind2, new_ids2)):
            if np.random.rand() < indp:
                if poolsize < 1:
                    raise ValueError("mate: the candidate pool is empty (poolsize = 0)")
                val = pool.distances(pair, new_ids)[0].sum(axis=0)           # distance to parent 1 + distance to parent 2
                ind[0] = new_ids[_pick(val, np.argsort(val, kind="stable"), oneofkbest, "mate")]
    else:
        for i in range(len(ind1)):
            if np.random.rand() < indp:
                ind1[i], ind2[i] = ind2[i], ind1[i]
    return ind1, ind2


def replace_individuals_randomly(individuals, pool: OEPool):
    """`evolve/__init__.py:160-164`, as written there: every ENTRY of the list becomes a random OE id"""
    for n in range(len(individuals)):
        individuals[n] = int(np.random.randint(0, len(pool.valid_indices)))
    return individuals


def select_individual(individuals, k: int, tournsize: int, fit_attr: str = "fitness", replace: bool = False) -> list:
    """tournament selection (`evolve/__init__.py:167-185`): k survivors, each the best of `tournsize` random aspirants; whether
    "best" is the largest or the smallest value is the individuals' fitness weight"""
    chosen = []
    for _ in range(k):
        aspirants = [individuals[i] for i in np.random.choice(len(individuals), tournsize, replace)]
        chosen.append(max(aspirants, key=lambda a: getattr(a, fit_attr)))
    return chosen


# ------------------------------------------------------------------------------------------------------------------ driver
class Toolbox:
    """the bound operators of one experiment (DEAP's toolbox in the reference)"""

    def __init__(self, **fns):
        self.__dict__.update(fns)

    clone = staticmethod(deepcopy)


def _history(setup: dict) -> dict:
    return {"pop": [], "fit": [], "mean_fit": [], "std_fit": [], "max_fit": [], "min_fit": [], "setup": setup}


def _population(pool: OEPool, oesize: int, generation_pool: int, weight: float, tree: Genealogy) -> list:
    pop = [Individual([init_individual(pool) for _ in range(oesize)], weight) for _ in range(generation_pool)]
    for ind in pop:
        tree.add(ind)
    return pop


def evolve_setup(oesize: int, generation_pool: int, mutation_pool: int, mutation_indp: float, mutation_oneofkbest: int,
                 mutation_chance: float, mate_chance: float, generations: int, select_toursize: int, pool: OEPool,
                 evaluate_fn: Callable, oeds: str = None, maxfit: bool = True):
    """`main/__init__.py:366-430`: (first population, 0, toolbox, history, genealogy).  The history's keys are the reference's,
    spelled as there ('geneation_pool')"""
    history = _history({
        "oesize": oesize, "geneation_pool": generation_pool, "mutation_pool": mutation_pool, "mutation_indp": mutation_indp,
        "mutation_oneofkbest": mutation_oneofkbest, "mutation_chance": mutation_chance, "mate_chance": mate_chance,
        "generations": generations, "oeds": oeds, "select_toursize": select_toursize})
    toolbox = Toolbox(
        evaluate=evaluate_fn,
        mate=lambda a, b: mate_individuals(a, b, pool, mutation_pool, mutation_indp, mutation_oneofkbest),
        mutate=lambda a: mutate_individual(a, pool, mutation_pool, mutation_indp, mutation_oneofkbest),
        select=lambda pop, k: select_individual(pop, k, tournsize=select_toursize))
    tree = Genealogy()
    pop = _population(pool, oesize, generation_pool, 1.0 if maxfit else -1.0, tree)
    return pop, 0, toolbox, history, tree


def rand_pick_setup(oesize: int, generation_pool: int, pool: OEPool, evaluate_fn: Callable, maxfit: bool = True):
    """`main/__init__.py:433-482`: `generation_pool` random OE subsets to evaluate once, no evolution"""
    history = _history({"oesize": oesize})
    toolbox = Toolbox(
        evaluate=evaluate_fn,
        mate=lambda a, b: mate_individuals(a, b, pool, 0, 0.0, 0),
        mutate=lambda a: mutate_individual(a, pool, 0, 0.0, 0),
        select=lambda pop, k=None: replace_individuals_randomly(pop, pool))
    tree = Genealogy()
    pop = _population(pool, oesize, generation_pool, 1.0 if maxfit else -1.0, tree)
    return pop, 0, toolbox, history, tree


def _flat_ids(individuals) -> list:
    return [int(i) for ind in individuals for i in ind]


def _stage_figure(logger, pool: OEPool, name: str, before: list, after: list, groups: list, flat: bool = False):
    """a selection / mating / mutation figure (`evolve/__init__.py:278-355`): the id lists `before` over the id lists `after`, one
    individual per row (one image each: all in one row) with 16 black rows between the two, and every group of individuals in
    `groups` (positions in before + after) framed in a colour of its own.  `flat` is the selection figure's rule for several
    images per individual (:285): ONE flat list of cells, so that every cell takes the next colour"""
    size = len(before[0])
    if size > 1:
        nrow, row_sep_at = size, (16, len(before))
        mark = [[j for i in group for j in range(i * size, (i + 1) * size)] for group in groups]
        mark = [j for group in mark for j in group] if flat else mark
    else:
        nrow, row_sep_at, mark = len(before), (16, 1), groups
    return logger.logimg(name, pool, _flat_ids(before) + _flat_ids(after), nrow=nrow, row_sep_at=row_sep_at, mark=mark)


def evaluate(offspring: list, pop: list, gen: int, toolbox: Toolbox, history: dict, tree: Genealogy, logger=None, pool: OEPool = None,
             log_images: bool = False):
    """`evolve/__init__.py:188-249`: train every offspring whose fitness is unset, make the offspring the population and append
    the generation's statistics to the history.  `log_images` (needs `logger` and `pool`): the picture of every newly evaluated
    individual as `individuals/gen{g}_ind{i}_fit{f}` (its path goes to the individual's genealogy node), the generation as
    `raw_gen/gen{g}` and, individuals ordered by fitness, as `gen{g}` with the fitness values as row headers"""
    if log_images and (logger is None or pool is None):
        raise ValueError("log_images needs a logger (logimg) and the OE pool")
    for i, ind in enumerate(offspring):
        if ind.fitness.valid:
            continue
        if logger is not None:
            logger.print(f"Evaluate ind{i:03}..")
        fit = float(toolbox.evaluate(ind))
        ind.fitness.values = (fit,)
        name, file = f"gen{gen:03}_ind{i:03}_fit{fit * 100:06.3f}", None
        if log_images:
            logger.logimg(os.path.join("individuals", name), pool, list(ind), nrow=16)
            file = os.path.join(logger.dir or "", "individuals", name + ".png")
        tree.evaluated(ind, gen, fit, file)
        if logger is not None:
            logger.logtxt(f"{name} with ids {list(ind)}")
    pop[:] = offspring
    fits = [ind.fitness.values[0] for ind in pop]
    history["pop"].append([[int(i) for i in ind] for ind in pop])
    history["fit"].append(fits)
    history["mean_fit"].append(float(np.mean(fits)))
    history["std_fit"].append(float(np.std(fits)))
    history["min_fit"].append(float(np.min(fits)))
    history["max_fit"].append(float(np.max(fits)))
    if log_images:
        logger.logimg(os.path.join("raw_gen", f"gen{gen:03}"), pool, _flat_ids(pop), nrow=len(pop[0]))
        order = sorted(range(len(pop)), key=lambda i: fits[i])
        logger.logimg(f"gen{gen:03}", pool, _flat_ids(pop[i] for i in order), nrow=len(pop[0]),
                      rowheaders=[f"{fits[i] * 100:06.3f}" for i in order])
    if logger is not None:
        logger.print(f"GENERATION {gen:03}")
        logger.print(f"  Min {history['min_fit'][-1] * 100:06.3f}")
        logger.print(f"  Max {history['max_fit'][-1] * 100:06.3f}")
        logger.print(f"  Avg {history['mean_fit'][-1] * 100:06.3f}")
        logger.print(f"  Std {history['std_fit'][-1] * 100:06.3f}")


def evolve(pop: list, gen: int, toolbox: Toolbox, mate_chance: float, mutation_chance: float, history: dict, tree: Genealogy,
           logger=None, pool: OEPool = None, log_images: bool = False):
    """one generation (`evolve/__init__.py:252-357`): tournament survivors, neighbours mated with `mate_chance`, everyone
    mutated with `mutation_chance` (both drawn from `random`, as there), then `evaluate`.  `log_images`: `selection/gen{g}`,
    `mating/gen{g}` and `mutation/gen{g}` show the population in front of and behind each stage, with the survivors, the mated
    pairs and the mutants framed (`:278-355`); no draw depends on it"""
    if log_images and (logger is None or pool is None):
        raise ValueError("log_images needs a logger (logimg) and the OE pool")
    n = len(pop)

    def figure(stage, before, groups, flat=False):
        if log_images:
            _stage_figure(logger, pool, os.path.join(stage, f"gen{gen:03}"), before, offspring, groups, flat)

    offspring = [toolbox.clone(ind) for ind in toolbox.select(pop, len(pop))]
    figure("selection", pop, [[i for i, ind in enumerate(pop) if ind in offspring]] if log_images else None, flat=True)
    before, picked = [list(ind) for ind in offspring] if log_images else None, []
    for i, (child1, child2) in enumerate(zip(offspring[::2], offspring[1::2])):
        if random.random() < mate_chance:
            parents = (child1.node, child2.node)
            toolbox.mate(child1, child2)
            picked.append(i)
            for child in (child1, child2):
                child.fitness.invalidate()
                tree.add(child, parents)
    figure("mating", before, [[p * 2, p * 2 + 1, n + p * 2, n + p * 2 + 1] for p in picked])
    before, picked = [list(ind) for ind in offspring] if log_images else None, []
    for i, mutant in enumerate(offspring):
        if random.random() < mutation_chance:
            parent = mutant.node
            toolbox.mutate(mutant)
            picked.append(i)
            mutant.fitness.invalidate()
            tree.add(mutant, (parent,))
    figure("mutation", before, [[p, n + p] for p in picked])
    evaluate(offspring, pop, gen, toolbox, history, tree, logger, pool, log_images)


def trainer_fitness(trainer, pool: OEPool, classes: Sequence[int], iterations: int) -> Callable:
    """the reference's `evaluate_individual` (`evolve/__init__.py:55-78`): the mean test AUC of `trainer.run(classes,
    iterations)` with the task's OE set restricted to the individual's images; the restriction is lifted again afterwards"""

    def fitness(ind) -> float:
        rows = [int(r) for r in pool.rows(list(ind))]
        kept = trainer.oe_limit_samples
        trainer.oe_limit_samples = rows                  # `trainer.oe_limit_samples = individual` (:70); run() applies it to trainer.ds
        try:
            return trainer.run(list(classes), iterations)[1]["mean_auc"]
        finally:
            trainer.oe_limit_samples = kept
            trainer.ds.set_oe_subset(None)

    return fitness


def prepare_trainer(trainer, classes: Sequence[int]):
    """`evolve_trainer` (`main/__init__.py:320-363`): the task's source is built ONCE and kept in `trainer.ds`, so that an
    individual's evaluation only swaps the OE subset.  More than one class is refused, as there (:352-358): `run` would build a
    fresh source per class and the individual's restriction would be lost."""
    if classes is None or len(classes) != 1:
        raise NotImplementedError("Atm, evolve for multiple classes at once does not work.")
    if trainer.ds is None:
        trainer.ds = trainer._task_source(int(classes[0]), 0)
    if not hasattr(trainer.ds, "set_oe_subset"):
        raise TypeError("the evolve driver needs a source whose OE set can be restricted (set_oe_subset), e.g. ResidentImageSource")
    return trainer.ds


def run_evolution(trainer, pool: Optional[OEPool], classes: Sequence[int], iterations: int = 1, *, oesize: int = 1,
                  generation_pool: int = 16, mutation_pool: int = 100, mutation_indp: float = 1.0, mutation_oneofkbest: int = 3,
                  mutation_chance: float = 0.5, mate_chance: float = 0.2, generations: int = 30, select_toursize: int = 3,
                  minimize_fitness: bool = False, fitness_fn: Callable = None, random_pick: bool = False,
                  log_images: bool = False) -> dict:
    """the evolve experiment (`main/evolve_oe_cifar.py:82-103`; `random_pick`: `main/random_oe_cifar.py:76-82`) with the
    reference's defaults.  `pool`: the OE images the ids name (None: the resident OE set of the trainer's source, which must be a
    tensor; for a ragged one pass `OEPool.from_source(trainer.ds)`).  `fitness_fn`
    (individual -> float) replaces the default, the mean test AUC of `trainer.run(classes, iterations)` on the individual's OE
    images; with it no trainer is needed (`trainer` may be None).  Returns the history; it is also written as
    `evolve_results.json` (the trainer's own `results.json` of the last training lies next to it), and the genealogy (node id,
    generation, ids, fitness, parent ids) as `evolution.json`, through the trainer's logger.

    `log_images=True` also writes the reference's figures through `logger.logimg`, each composed on the device from (pool, ids):
    per evaluated individual `individuals/gen{g}_ind{i}_fit{f}.png` (the path is kept on its genealogy node as `file`), per
    generation `raw_gen/gen{g}`, `gen{g}` (sorted by fitness), `selection/`, `mating/` and `mutation/gen{g}`, and at the end
    `final/best_raw`, `final/best`, `final/worst_raw`, `final/worst`.  Off (the default) nothing of it runs and the same files
    are written as before."""
    logger = getattr(trainer, "logger", None)
    if log_images and not hasattr(logger, "logimg"):
        raise ValueError("log_images=True needs the trainer's logger to have logimg (JsonLogger)")
    if fitness_fn is None:
        ds = prepare_trainer(trainer, classes)
        if pool is None:
            pool = OEPool(ds.oe)
        fitness_fn = trainer_fitness(trainer, pool, classes, iterations)
    elif pool is None:
        raise ValueError("an injected fitness function needs the OE pool to be given")
    if mutation_pool > RANK_MAX_CANDIDATES and pool.images.is_cuda:
        raise ValueError(f"mutation_pool of at most {RANK_MAX_CANDIDATES} candidates on the device path, not {mutation_pool}")
    if random_pick:
        pop, gen, toolbox, history, tree = rand_pick_setup(oesize, generation_pool, pool, fitness_fn, not minimize_fitness)
        generations = 1
    else:
        pop, gen, toolbox, history, tree = evolve_setup(
            oesize, generation_pool, mutation_pool, mutation_indp, mutation_oneofkbest, mutation_chance, mate_chance, generations,
            select_toursize, pool, fitness_fn, getattr(trainer, "oe_dsstr", None), not minimize_fitness)
    try:
        evaluate(pop, pop, gen, toolbox, history, tree, logger, pool, log_images)
        for gen in range(1, generations):
            evolve(pop, gen, toolbox, mate_chance, mutation_chance, history, tree, logger, pool, log_images)
        if log_images:
            tree.imsave_collection_best(logger, pool)
    finally:
        if logger is not None:
            logger.logjson("evolve_results", history)
            logger.logjson("evolution", tree.to_json())
    return history
