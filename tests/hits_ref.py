"""The reference of pt_trace_hits (include/mi355pt.h "ray queries: the first K hits"), independent of product code: everything here
comes from the oracle's brute-force closest hit (oracle.Scene.intersect(..., use_bvh=False), which takes tmin and tmax, t > tmin strictly).

CHAIN of a ray: level 0 = S.intersect(org, dir, 1e-3, thi); level j + 1 = the same call with tmin = t_j; it stops at a miss.  These are
the distinct t-levels of the definition's set S in order, each with the LOWEST id at its level - so the chain does not see the further
triangles of a tie.
REAL: an entry {t, u, v, prim} is real if a ONE-triangle oracle scene of tris[prim] returns exactly that t, u, v for the ray within
(1e-3, thi].

THE RULE for a list of K records (check_lists):
  * the hits come first and every record behind them is the miss record {+0, +0, +0, -1};
  * the hits are strictly ascending in (t, id);
  * collapsed to the first entry of each run of equal t, the list equals the chain bit for bit - for as many levels as K leaves room
    for; where K cuts the last run, its first entry is still compared;
  * every further entry of a run is REAL;
  * a list that is not full leaves the chain no level.
The rule needs no cap on skipped rays.  WHICH RAYS: ALL compared rays of every case (the battery's usual mask,
trace_rays_common.compared; every ray of the constructed scenes) - the chain is affordable: at most 24 000 triangles, about 15 000
rays and a handful of levels each, on a thread pool (the ctypes call releases the GIL).  No sampling is used.

MUTATIONS: deliberately wrong lists made from a right one (mutations), which the rule must reject.
WHAT THE RULE CANNOT SEE: the chain holds one triangle per t-level, so the rule does not know how many partners a tie has.  "A tie
partner dropped" is rejected here only because the shortened list is no longer full while the chain goes on; a partner missing from
a list that was not full anyway, or from a full list closed up with the next hit, passes the rule.  A lost partner is caught by
hits_common.doubled_expectation - the doubled stack's lists by construction, in the host and the GPU test - not by the rule."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from owl_path_tracer_amd.pyhost import binding as B

LEVELS = B.PT_HITS_MAX + 1  # levels of a chain that are computed: one more than the longest list, so "no level left" is decidable
K_TMIN = 1e-3
_MISS = np.array([0, 0, 0, 0xFFFFFFFF], np.uint32)


def _thi(tmax):
    t = np.float32(tmax)
    return float(t) if t < np.float32(1e10) else 1e10  # NaN and +inf: the library's bound


def chain(S, org, direction, tmax, levels=LEVELS):
    """The chain of one ray as an (m, 4) uint32 array of {t, u, v, prim} bits, m <= levels."""
    thi, tmin, out = _thi(tmax), K_TMIN, []
    while len(out) < levels:
        ok, t, u, v, p = S.intersect(org, direction, tmin=tmin, tmax=thi, use_bvh=False)
        if not ok:
            break
        out.append((np.float32(t).view(np.uint32), np.float32(u).view(np.uint32), np.float32(v).view(np.uint32), np.int32(p).view(np.uint32)))
        tmin = t
    return np.array(out, np.uint32).reshape(-1, 4)


def chains(S, rec, idx):
    """(chain, length) of the rays rec[idx]: (len(idx), LEVELS, 4) uint32 padded with miss records, and (len(idx),) levels found."""
    idx = np.asarray(idx)
    ch = np.tile(_MISS, (idx.size, LEVELS, 1))
    ln = np.zeros(idx.size, np.int32)

    def one(j):
        r = rec[idx[j]]
        c = chain(S, r["org"], r["dir"], r["tmax"])
        ch[j, :c.shape[0]] = c
        ln[j] = c.shape[0]

    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        list(pool.map(one, range(idx.size), chunksize=64))
    ch.setflags(write=False)
    ln.setflags(write=False)
    return ch, ln


class Real:
    """The REAL test against one-triangle oracle scenes, made on demand and kept."""

    def __init__(self, orc, tris, watertight=False):
        self.orc, self.tris, self.wt, self.scenes = orc, tris, watertight, {}

    def __call__(self, ray, entry):
        import ray_battery as rb

        prim = int(entry["prim"])
        if not 0 <= prim < self.tris.shape[0]:
            return False
        if prim not in self.scenes:
            self.scenes[prim] = rb.oracle_scene(self.orc, self.tris[prim:prim + 1])
            if self.wt:
                self.scenes[prim].set_watertight(True)
        ok, t, u, v, _ = self.scenes[prim].intersect(ray["org"], ray["dir"], tmin=K_TMIN, tmax=_thi(ray["tmax"]), use_bvh=False)
        got = np.float32([t, u, v]).view(np.uint32)
        want = np.array([entry["t"], entry["u"], entry["v"]], np.float32).view(np.uint32)
        return bool(ok) and bool((got == want).all())


def check_lists(lists, ch, ln, rays, real):
    """THE RULE on lists (n, K) HIT_DTYPE against the chains (ch, ln) of the same n rays (rays: their pt_ray records; real: a Real).
    Returns a list of (ray, reason) for the lists it rejects - empty: every list passes."""
    n, K = lists.shape
    bits = np.ascontiguousarray(lists).view(np.uint32).reshape(n, K, 4)
    t, prim = lists["t"], lists["prim"]
    bad = {}

    def reject(mask, why):
        for i in np.nonzero(mask)[0]:
            bad.setdefault(int(i), why)

    valid = prim >= 0
    nv = valid.sum(1)
    j = np.arange(K)[None, :]
    reject((valid != (j < nv[:, None])).any(1), "a hit behind a miss")
    reject((~valid & (bits != _MISS).any(2)).any(1), "a miss that is not {+0, +0, +0, -1}")
    pair = valid[:, 1:] & valid[:, :-1]
    asc = (t[:, :-1] < t[:, 1:]) | ((t[:, :-1] == t[:, 1:]) & (prim[:, :-1] < prim[:, 1:]))
    reject((pair & ~asc).any(1), "not strictly ascending in (t, id)")
    start = valid.copy()
    start[:, 1:] &= t[:, 1:] != t[:, :-1]
    run = np.cumsum(start, 1) - 1  # the level of the chain an entry belongs to
    runs = start.sum(1)
    reject((start & (run >= ln[:, None])).any(1), "a level the chain does not have")
    level = np.take_along_axis(ch, np.clip(run, 0, LEVELS - 1)[:, :, None], 1)  # (n, K, 4)
    reject((start & (bits != level).any(2)).any(1), "the first entry of a run is not the chain's level")
    reject((nv < K) & (ln != runs), "the list is not full and the chain has a level left")
    for i, k in zip(*np.nonzero(valid & ~start)):  # the further entries of a run: rare
        if int(i) not in bad and not real(rays[i], lists[i, k]):
            bad[int(i)] = "entry %d of a run is not real" % k
    return sorted(bad.items())


def assert_lists(lists, ch, ln, rays, real, what):
    bad = check_lists(lists, ch, ln, rays, real)
    if bad:
        i, why = bad[0]
        raise AssertionError("%s: the rule rejects %d of %d lists; first: ray %d, %s\n list %r\n chain %r (%d levels)\n ray %r" % (
            what, len(bad), lists.shape[0], i, why, lists[i], ch[i, :ln[i]].view(np.float32), ln[i], rays[i]))


def _shifted_out(lst, k):
    """lst without entry k: the entries behind it move up, a miss record closes the list."""
    out = lst.copy()
    out[k:-1] = lst[k + 1:]
    out[-1] = (0, 0, 0, -1)
    return out


def mutations(full_with_tie, at_thi, first):
    """Deliberately wrong lists, as (label, ray slot, list): `full_with_tie` = (list, k): a right FULL list whose chain goes on behind it,
    entry k being the second of a tie; `at_thi` = a right list of a ray whose last hit has t == thi exactly, with room behind it;
    `first` = any right list with a hit and room behind it.  The slot says which of the three rays the list is to be checked against."""
    lst, k = full_with_tie
    assert lst["prim"][-1] >= 0 and lst["t"][k] == lst["t"][k - 1]
    swapped = lst.copy()
    swapped[[0, 1]] = lst[[1, 0]]
    tie_swapped = lst.copy()
    tie_swapped[[k - 1, k]] = lst[[k, k - 1]]
    n_at = int((at_thi["prim"] >= 0).sum())
    assert 0 < n_at < at_thi.shape[0]
    dropped_at_thi = at_thi.copy()
    dropped_at_thi[n_at - 1] = (0, 0, 0, -1)
    assert first["prim"][0] >= 0 and first["prim"][-1] < 0
    below = first.copy()
    below[1:] = first[:-1]
    below[0] = (np.float32(5e-4), first["u"][0], first["v"][0], first["prim"][0])  # a hit with t <= 1e-3 kept in front
    return [("a tie partner dropped", 0, _shifted_out(lst, k)), ("two entries swapped", 0, swapped), ("the two partners of a tie swapped", 0, tie_swapped),
            ("a hit at exactly thi dropped", 1, dropped_at_thi), ("a hit with t <= 1e-3 kept", 2, below)]
