"""Plain numpy references of the two device BVH builders (csrc/pt_lbvh.hip), written from the definitions in that file's header
comments, and the canonical form in which a reference tree and a context's export are compared.  Shared by
tests/test_builder_ref_host.py (CPU: the references held to their own definitions) and tests/test_gpu_builders.py (the device).

The library is compiled with -ffp-contract=off -fno-fast-math: every float32 expression of a kernel has one value, and numpy gives
the same one when every intermediate is a float32 in the order the source writes it.  Finite input only.

KEYS      centroid ((p0 + p1) + p2) * f32(1/3); per axis t = (c - lo) / ext over the centroid bounds, 0 where ext <= 0; cell
          trunc(clamp(t * 1024, 0, 1023)); 30-bit Morton code, x in the highest bit of each triple; key = code << 32 | index.
LBVH      the keys sorted; a range splits at the highest bit in which its first and last key differ; a range of at most leaf_size
          triangles is one leaf, triangles in sorted order.
PLOC      clusters in key order; per round cluster i takes the j in [i - r, i + r], j != i, of the smallest
          ((dx * dy) + (dy * dz)) + (dz * dx) of the union box, the first j on a tie; mutual pairs merge into a node (lower position,
          higher position) at the lower position; then the rules of pt_bvh_from_hierarchy: a subtree of at most leaf_size triangles
          is a leaf, depth first with the left child first.
BOXES     a node stores, per child, the exact min / max of the vertices below it, then one float32 - pad / + pad, with
          pad = f32(1e-5) * max over the axes of (hi - lo, |lo|, |hi|) of the vertex bounds.
DEPTH     internal nodes on the deepest chain, counted from 1.

CANONICAL FORM  pre-order list: ("N", bytes of the two child boxes) per node, ("L", ordered tuple of real triangle ids) per leaf.
Node numbers and padding slots drop out - all that pt_bvh_layout changes, and all that the atomicAdd of the PLOC merge decides.
"""
import bisect
import json
import os

import numpy as np

F32 = np.float32
PAD_SLOT = 0x7fffffff
PLOC_ROUND_CAP = 4096  # pt_ploc_build_device gives up after this many rounds and the host builder takes over
DEFAULT_MAX_DEPTH = 48  # option max_bvh_depth
DEFAULT_RADIUS = 16  # option ploc_radius
MAX_STACK = 64  # PT_MAX_STACK
GOLDEN_ROUNDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ploc_strip_rounds.json")


# ---------------------------------------------------------------------------------------------------------------------
# input: the context's own triangle records
# ---------------------------------------------------------------------------------------------------------------------
def positions_of(ex):
    """(n, 3, 3) float32 indexed by triangle id, from an export's leaf-ordered records (the sliver rule of the upload applied)."""
    t = ex["tris"]
    real = t["id"] != PAD_SLOT
    n = int(real.sum())
    P = np.zeros((n, 3, 3), np.float32)
    P[t["id"][real]] = np.stack([t["p0"][real], t["p1"][real], t["p2"][real]], 1)
    return P


def scene_pad(P):
    v = P.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    ext = F32(0)
    for a in range(3):
        ext = max(ext, F32(hi[a] - lo[a]))
        ext = max(ext, max(abs(lo[a]), abs(hi[a])))
    return F32(F32(ext) * F32(1e-5))


def centroids(P):
    return ((P[:, 0] + P[:, 1]) + P[:, 2]) * (F32(1) / F32(3))


def cells(P):
    """(n, 3) uint32 grid cells of the centroids."""
    c = centroids(P)
    lo, hi = c.min(0), c.max(0)
    ext = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ext > 0, (c - lo) / ext, F32(0)).astype(np.float32)
    return np.trunc(np.clip(t * F32(1024), F32(0), F32(1023))).astype(np.uint32)


def morton_keys(P):
    """Python ints code << 32 | index, in triangle order."""
    q = cells(P).astype(np.uint64)
    code = np.zeros(P.shape[0], np.uint64)
    for b in range(10):
        for a in range(3):  # x highest in each triple
            code |= ((q[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - a)
    return [(int(c) << 32) | i for i, c in enumerate(code)]


def tri_boxes(P):
    return P.min(1), P.max(1)


# ---------------------------------------------------------------------------------------------------------------------
# a binary hierarchy over sorted triangles -> canonical form (the leaf rule and the depth rule are the same for both builders)
# ---------------------------------------------------------------------------------------------------------------------
class Hierarchy:
    """Nodes 0 .. n - 1 are the triangles in key order (`order`: position -> triangle id), nodes >= n are internal."""

    def __init__(self, order, lo, hi):
        self.n = len(order)
        self.order = [int(x) for x in order]
        self.left, self.right = [-1] * self.n, [-1] * self.n
        self.count = [1] * self.n
        self.lo, self.hi = [r for r in lo], [r for r in hi]
        self.root = -1
        self.rounds = 0
        self.range = {}  # LBVH only: internal node -> (first, last) sorted position

    def add(self, l, r):
        self.left.append(l)
        self.right.append(r)
        self.count.append(self.count[l] + self.count[r])
        self.lo.append(np.minimum(self.lo[l], self.lo[r]))
        self.hi.append(np.maximum(self.hi[l], self.hi[r]))
        return len(self.left) - 1

    def leaf_ids(self, p):
        out, st = [], [p]
        while st:
            q = st.pop()
            if q < self.n:
                out.append(self.order[q])
            else:
                st += [self.right[q], self.left[q]]
        return tuple(out)


class RefTree:
    def __init__(self, form, pad, depth, max_leaf):
        self.form, self.pad, self.depth, self.max_leaf = form, F32(pad), int(depth), int(max_leaf)
        self.n_nodes = sum(1 for e in form if e[0] == "N")

    def too_deep(self, max_depth, builder):
        """Whether build_bvh hands this tree over to the host builder."""
        lim = min(max_depth, MAX_STACK) if builder == 1 else max(2, min(MAX_STACK, max_depth))
        return self.depth > lim


def _box_bytes(llo, lhi, rlo, rhi, pad):
    return np.concatenate([llo - pad, lhi + pad, rlo - pad, rhi + pad]).astype(np.float32).tobytes()


def layout(h, leaf_size, pad):
    """Canonical form of hierarchy h under the leaf rule."""
    leaf_size = max(1, min(7, leaf_size))
    form, depth, max_leaf = [], 0, 0
    st = [(h.root, 1)]
    while st:
        p, d = st.pop()
        if h.count[p] <= leaf_size:
            form.append(("L", h.leaf_ids(p)))
            max_leaf = max(max_leaf, h.count[p])
            continue
        depth = max(depth, d)
        l, r = h.left[p], h.right[p]
        form.append(("N", _box_bytes(h.lo[l], h.hi[l], h.lo[r], h.hi[r], pad)))
        st += [(r, d + 1), (l, d + 1)]
    return RefTree(form, pad, depth, max_leaf)


def form_of_export(ex):
    """Canonical form of a context's binary tree (Context.export_trees)."""
    nd, tr = ex["nodes"], ex["tris"]
    ids = tr["id"]
    form = []
    st = [int(ex["root"])]
    while st:
        r = st.pop()
        if r < 0:
            code = ~r & 0xffffffff
            first, count = code >> 3, code & 7
            form.append(("L", tuple(int(i) for i in ids[first:first + count] if i != PAD_SLOT)))
            continue
        n = nd[r]
        form.append(("N", np.concatenate([n["lo"][:, 0], n["hi"][:, 0], n["lo"][:, 1], n["hi"][:, 1]]).astype(np.float32).tobytes()))
        st += [int(n["right"]), int(n["left"])]
    return form


def same_tree(ex, ref):
    """Equality as the tests mean it: the canonical form, pad bit for bit, depth and max_leaf.  Returns a description of the first
    difference, or None."""
    if F32(ex["pad"]).tobytes() != F32(ref.pad).tobytes():
        return "pad %r, reference %r" % (float(ex["pad"]), float(ref.pad))
    if (ex["depth"], ex["max_leaf"]) != (ref.depth, ref.max_leaf):
        return "depth %d max_leaf %d, reference %d %d" % (ex["depth"], ex["max_leaf"], ref.depth, ref.max_leaf)
    got = form_of_export(ex)
    if got == ref.form:
        return None
    if len(got) != len(ref.form):
        return "%d entries, reference %d" % (len(got), len(ref.form))
    k = next(i for i, (a, b) in enumerate(zip(got, ref.form)) if a != b)
    show = lambda e: e[1] if e[0] == "L" else np.frombuffer(e[1], np.float32).tolist()
    return "entry %d in pre-order: %s %r, reference %s %r" % (k, got[k][0], show(got[k]), ref.form[k][0], show(ref.form[k]))


# ---------------------------------------------------------------------------------------------------------------------
# LBVH
# ---------------------------------------------------------------------------------------------------------------------
def sorted_keys(P):
    keys = sorted(morton_keys(P))
    return keys, [k & 0xffffffff for k in keys]


def lbvh_hierarchy(P):
    """The binary radix tree over the sorted keys, down to single triangles."""
    keys, order = sorted_keys(P)
    tlo, thi = tri_boxes(P)
    h = Hierarchy(order, tlo[order], thi[order])

    def build(first, last):
        if first == last:
            return first
        bit = (keys[first] ^ keys[last]).bit_length() - 1  # the highest bit in which the two ends differ
        split = bisect.bisect_left(keys, (keys[last] >> bit) << bit, first, last + 1)  # first key with that bit set
        l, r = build(first, split - 1), build(split, last)
        p = h.add(l, r)
        h.range[p] = (first, last)
        return p

    h.root = build(0, h.n - 1)
    h.keys = keys
    return h


def lbvh_reference(P, leaf_size, h=None):
    return layout(h or lbvh_hierarchy(P), leaf_size, scene_pad(P))


def karras_hierarchy(P):
    """The same tree by the second formulation: Karras 2012, section 4 - every internal node i in 0 .. n - 2 finds its own range and
    split from common-prefix lengths delta(i, j), with no recursion over ranges.  Plain Python: small inputs only."""
    keys, order = sorted_keys(P)
    n = len(keys)
    tlo, thi = tri_boxes(P)

    def delta(i, j):
        return -1 if j < 0 or j >= n else 64 - (keys[i] ^ keys[j]).bit_length()

    kids, rng = {}, {}
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, l
        while t > 1:
            t = (t + 1) // 2
            if delta(i, i + (s + t) * d) > dnode:
                s += t
        gamma = i + s * d + min(d, 0)
        first, last = min(i, j), max(i, j)
        kids[i] = (("leaf", gamma) if first == gamma else ("node", gamma), ("leaf", gamma + 1) if last == gamma + 1 else ("node", gamma + 1))
        rng[i] = (first, last)
    h = Hierarchy(order, tlo[order], thi[order])
    made = {}
    todo = [0]
    while todo:  # children before parents
        i = todo[-1]
        need = [c[1] for c in kids[i] if c[0] == "node" and c[1] not in made]
        if need:
            todo += need
            continue
        todo.pop()
        l, r = (c[1] if c[0] == "leaf" else made[c[1]] for c in kids[i])
        made[i] = h.add(l, r)
        h.range[made[i]] = rng[i]
    h.root = made[0]
    h.keys = keys
    return h


# ---------------------------------------------------------------------------------------------------------------------
# PLOC
# ---------------------------------------------------------------------------------------------------------------------
def _nearest(lo, hi, radius):
    """For every cluster position the position of its nearest neighbour (-1: none)."""
    m = lo.shape[0]
    r = min(radius, m - 1)
    cand = np.full((m, 2 * r), np.inf, np.float32)  # columns: j = i - r .. i - 1, i + 1 .. i + r
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(1, r + 1):
            e = np.maximum(hi[:-d], hi[d:]) - np.minimum(lo[:-d], lo[d:])  # union box of i and i + d: one extent per axis
            a = ((e[:, 0] * e[:, 1]) + (e[:, 1] * e[:, 2])) + (e[:, 2] * e[:, 0])
            cand[:m - d, r + d - 1] = a
            cand[d:, r - d] = a
    col = np.argmin(cand, 1)  # the first smallest: the lowest j
    off = np.where(col < r, col - r, col - r + 1)
    best = cand[np.arange(m), col]
    return np.where(best < np.inf, np.arange(m) + off, -1)


def ploc_hierarchy(P, radius, trace=None):
    """The PLOC hierarchy; `rounds` counts the rounds.  trace: a list that receives (cluster nodes, nn, merged lower positions) of
    every round."""
    keys, order = sorted_keys(P)
    tlo, thi = tri_boxes(P)
    h = Hierarchy(order, tlo[order], thi[order])
    cid = np.arange(h.n)
    lo, hi = tlo[order].copy(), thi[order].copy()
    while cid.size > 1:
        nn = _nearest(lo, hi, radius)
        i = np.arange(cid.size)
        mutual = (nn >= 0) & (nn[np.maximum(nn, 0)] == i)
        low = np.nonzero(mutual & (i < nn))[0]
        assert low.size, "a round without a mutual pair"
        if trace is not None:
            trace.append((cid.copy(), nn, low))
        keep = np.ones(cid.size, bool)
        for a in low:
            b = int(nn[a])
            cid[a] = h.add(int(cid[a]), int(cid[b]))
            keep[b] = False
        lo[low], hi[low] = np.minimum(lo[low], lo[nn[low]]), np.maximum(hi[low], hi[nn[low]])
        cid, lo, hi = cid[keep], lo[keep], hi[keep]
        h.rounds += 1
    h.root = int(cid[0])
    return h


def ploc_reference(P, leaf_size, radius=DEFAULT_RADIUS, h=None):
    return layout(h or ploc_hierarchy(P, radius), leaf_size, scene_pad(P))


def ploc_rounds(P, radius=DEFAULT_RADIUS):
    """Rounds only: the boxes without the hierarchy (the strip of the round-cap test needs thousands of rounds)."""
    _, order = sorted_keys(P)
    tlo, thi = tri_boxes(P)
    lo, hi = tlo[order].copy(), thi[order].copy()
    rounds = 0
    while lo.shape[0] > 1:
        nn = _nearest(lo, hi, radius)
        i = np.arange(lo.shape[0])
        low = np.nonzero((nn >= 0) & (nn[np.maximum(nn, 0)] == i) & (i < nn))[0]
        assert low.size
        keep = np.ones(lo.shape[0], bool)
        keep[nn[low]] = False
        lo[low], hi[low] = np.minimum(lo[low], lo[nn[low]]), np.maximum(hi[low], hi[nn[low]])
        lo, hi = lo[keep], hi[keep]
        rounds += 1
    return rounds


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_builders.py (test_builder_ref_host.py computes their reference figures and asserts what makes them
# meaningful: a device tree is expected where the reference is shallow enough, a fallback where it lies beyond its limit)
# ---------------------------------------------------------------------------------------------------------------------
LEAF_SIZES = (1, 4, 7)
RADII = (1, 16, 64)
FALLBACK_DEPTH = 14  # test 3: the Cornell box under max_bvh_depth = 14
STRIP_N = 9000  # test 4: ray_battery.strip_scene(STRIP_N) under bvh_builder = 2


def _soup(n, seed=20261017, size=0.05):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n, 1, 3))
    return (c + rng.normal(0, size, (n, 3, 3))).astype(np.float32)


def _grid():
    """Small triangles on a 6 x 6 x 6 grid, every triangle stored three times: duplicate codes and exact area ties."""
    g = np.arange(6, dtype=np.float32) * F32(0.25)
    c = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 1, 3)
    t = c + np.float32([[0, 0, 0], [0.125, 0, 0], [0, 0.125, 0.0625]])
    return np.repeat(t, 3, axis=0).astype(np.float32)


def _one_centroid(n=300):
    """p0 = a, p1 = b, p2 = -(a + b) with a, b small integers / 64: every sum is exact and every centroid is +0."""
    rng = np.random.default_rng(7)
    a, b = rng.integers(-64, 65, (2, n, 3))
    bad = (np.cross(a, b) == 0).all(1)
    a[bad], b[bad] = (1, 0, 0), (0, 1, 0)
    return (np.stack([a, b, -(a + b)], 1) / 64.0).astype(np.float32)


def _zeros(n=120):
    """Centroid coordinates of -0.0 and +0.0: x is -0.0 on every vertex of every third triangle and +0.0 on the others (ext == 0
    there); y is -0.0 on every vertex of a few triangles while the others lie above."""
    t = _soup(n, 5, 0.2)
    t[:, :, 0] = 0.0
    t[::3, :, 0] = -0.0
    t[:, :, 1] = np.abs(t[:, :, 1])
    t[::7, :, 1] = -0.0
    t[3::7, :, 1] = 0.0
    return t


def level_strip(n):
    """A strip of n triangles of equal width: every cluster's two neighbours tie, the first wins, so every cluster looks to its left
    and a single pair is mutual per round - about n / 2 rounds.  (The sliver strip of ray_battery.strip_scene does the same while its
    widths grow strictly; from x ~ 2^16 on float32 rounds them into a jitter in which many pairs are mutual at once, and its round
    count levels off below the cap: 4 088 rounds at 9 000 triangles, 4 091 at 12 000, 4 095 at 20 000.)"""
    x = np.arange(n + 1, dtype=np.float32)
    v = np.stack([np.stack([x, 0 * x, 0 * x], 1), np.stack([x, 0 * x + 1, 0 * x], 1)], 1).reshape(-1, 3)
    idx = np.array([[2 * i, 2 * i + 2, 2 * i + 1] for i in range(n)], np.int32)
    return v[idx].astype(np.float32)


def form_digest(form, pad, depth, max_leaf):
    """sha256 of a canonical form with pad, depth and max_leaf: what tests/golden/ploc_strip_rounds.json records of a reference tree
    that takes several seconds to compute."""
    import hashlib

    d = hashlib.sha256()
    d.update(F32(pad).tobytes() + np.int32([depth, max_leaf]).tobytes())
    for kind, body in form:
        d.update(kind.encode() + (body if kind == "N" else np.int32(body).tobytes()))
    return d.hexdigest()


def scene_cases(leaf_size):
    """name -> (n, 3, 3) float32, for one leaf size (one case has leaf_size + 1 triangles)."""
    import ray_battery as rb

    s = _soup(2000)
    out = {"n2": s[:2], "n3": s[:3], "leaf+1": s[10:10 + leaf_size + 1]}
    for n in (255, 256, 257, 513):
        out["n%d" % n] = _soup(n, 100 + n)
    out["soup2000"] = s
    out["grid_x3"] = _grid()
    out["one_centroid"] = _one_centroid()
    planar = _soup(200, 3, 0.1)
    planar[:, :, 2] = 0.5
    out["planar"] = planar
    out["negative"] = (_soup(300, 4, 0.1) - F32(5)).astype(np.float32)
    out["zeros"] = _zeros()
    out["offset30"] = rb.make_scene("soup_offset30")
    out["cornell"] = rb.make_scene("cornell")
    return out


CASE_NAMES = ("n2", "n3", "leaf+1", "n255", "n256", "n257", "n513", "soup2000", "grid_x3", "one_centroid", "planar", "negative", "zeros", "offset30", "cornell")


def combos(builder):
    """(leaf_size, radius) of a case under a builder: every leaf size at the default radius; for PLOC also radius 1 and 64 at leaf 4."""
    out = [(leaf, DEFAULT_RADIUS) for leaf in LEAF_SIZES]
    if builder == 2:
        out += [(4, r) for r in RADII if r != DEFAULT_RADIUS]
    return out


def host_export(tris, leaf_size=4, builder=0, max_depth=None, radius=None):
    """Export of a host-only context (always the host SAH builder's tree)."""
    import ray_battery as rb
    from owl_path_tracer_amd.pyhost import binding as B

    ctx = B.Context(-1)
    try:
        ctx.set_option("bvh_builder", builder)
        ctx.set_option("leaf_size", leaf_size)
        if max_depth is not None:
            ctx.set_option("max_bvh_depth", max_depth)
        if radius is not None:
            ctx.set_option("ploc_radius", radius)
        rb.upload(ctx, tris)
        return ctx.export_trees()
    finally:
        ctx.close()


_hier = {}


def reference(P, builder, leaf_size, radius=DEFAULT_RADIUS):
    """Reference tree for positions P; the hierarchy (independent of the leaf size) is computed once per (P, builder, radius)."""
    key = (P.shape[0], hash(P.tobytes()), builder, radius if builder == 2 else 0)
    if key not in _hier:
        _hier[key] = lbvh_hierarchy(P) if builder == 1 else ploc_hierarchy(P, radius)
    return layout(_hier[key], leaf_size, scene_pad(P)), _hier[key]


def export_bytes(ex):
    """Everything an export holds, as one comparable tuple."""
    return tuple((k, ex[k].tobytes() if isinstance(ex[k], np.ndarray) else (F32(ex[k]).tobytes() if k == "pad" else ex[k])) for k in sorted(ex))


def golden_rounds():
    with open(GOLDEN_ROUNDS) as fh:
        return json.load(fh)


PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r12_device_builders.json")


def write_profile(section, doc):
    if os.environ.get("PT_WRITE_PROFILES") != "1":
        return
    whole = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            whole = json.load(fh)
    whole[section] = doc
    with open(PROFILE, "w") as fh:
        json.dump(whole, fh, indent=1, sort_keys=True)
