"""The numpy references of the device BVH builders (tests/builder_ref.py) held to their own definitions - no GPU.

tests/test_gpu_builders.py compares csrc/pt_lbvh.hip with these references bit for bit; this file is what that comparison rests on:

* LBVH reference: every triangle in exactly one leaf, every box the exact union below it (one float32 -/+ pad), every internal range
  with a strictly longer common key prefix than its parent and split where that bit changes; and the same tree as a second
  formulation - Karras' per-node range and split search in plain Python - on the small cases.
* PLOC reference: in every round the nearest neighbours equal those of a plain double loop; each merged pair is mutual and no unmerged
  cluster had a mutual partner; radius >= m is an unbounded search.  Its layout passes the same leaf and box checks.
* A host-only context with bvh_builder 1 or 2 holds the tree of builder 0, byte for byte.
* The case table of the GPU tests with reference depth and rounds per case: every "device tree expected" case has more than
  leaf_size triangles, reference depth <= 48 and at most 4096 rounds; every "fallback expected" case lies beyond its limit.  The two
  strips of the round-cap test are computed here (~6 s each) and compared with what tests/golden/ploc_strip_rounds.json records, which
  the GPU test reads.

PT_WRITE_PROFILES=1 writes the table to profiles/r12_device_builders.json, section "reference".
"""
import time

import numpy as np
import pytest

import builder_ref as br
import ray_battery as rb

F32 = np.float32
SMALL = ("n2", "n3", "leaf+1", "n255", "n257", "one_centroid", "planar", "zeros", "offset30")

_pos = {}


def positions(name, leaf=4):
    """The case's positions as a context exports them (host-only context: the records do not depend on the builder)."""
    key = (name, leaf if name == "leaf+1" else 0)
    if key not in _pos:
        _pos[key] = br.positions_of(br.host_export(br.scene_cases(leaf)[name], leaf))
    return _pos[key]


def parse(form):
    """Pre-order list -> nested (kind, body, left, right)."""
    it = iter(form)

    def node():
        kind, body = next(it)
        return (kind, body, None, None) if kind == "L" else (kind, body, node(), node())

    root = node()
    assert next(it, None) is None
    return root


def check_layout(P, tree):
    """Every triangle in exactly one leaf; every stored box the exact vertex union of its subtree, then one float32 -/+ pad."""
    pad = br.scene_pad(P)
    assert tree.pad.tobytes() == pad.tobytes()
    seen = np.zeros(P.shape[0], np.int32)
    depth = [0]

    def below(t, d):
        kind, body, l, r = t
        if kind == "L":
            assert 1 <= len(body) <= tree.max_leaf
            np.add.at(seen, list(body), 1)
            return list(body)
        depth[0] = max(depth[0], d)
        il, ir = below(l, d + 1), below(r, d + 1)
        want = []
        for ids in (il, ir):
            v = P[ids].reshape(-1, 3)
            want += [v.min(0) - pad, v.max(0) + pad]
        assert np.concatenate(want).astype(np.float32).tobytes() == body, "a box is not the padded union of its subtree"
        return il + ir

    below(parse(tree.form), 1)
    assert (seen == 1).all()
    assert depth[0] == tree.depth


@pytest.mark.parametrize("name", br.CASE_NAMES)
def test_lbvh_reference_definition(name):
    for leaf in br.LEAF_SIZES:
        P = positions(name, leaf)
        h = br.lbvh_hierarchy(P)
        keys = h.keys
        assert keys == sorted(keys) and len(set(keys)) == P.shape[0] and all(k >> 62 == 0 for k in keys)
        check_layout(P, br.layout(h, leaf, br.scene_pad(P)))
        if leaf != br.LEAF_SIZES[0]:
            continue
        # the radix tree itself: ranges nest, a node splits where the first differing bit of its ends changes, prefixes grow strictly
        prefix = lambda f, l: 64 - (keys[f] ^ keys[l]).bit_length()
        rng = lambda p: h.range[p] if p >= h.n else (p, p)
        assert h.range[h.root] == (0, h.n - 1) or h.n == 1
        for p, (f, l) in h.range.items():
            (lf, ll), (rf, rl) = rng(h.left[p]), rng(h.right[p])
            assert lf == f and rl == l and ll + 1 == rf
            bit = 63 - prefix(f, l)
            assert all(not (keys[i] >> bit) & 1 for i in range(lf, ll + 1)) and all((keys[i] >> bit) & 1 for i in range(rf, rl + 1))
            for c in (h.left[p], h.right[p]):
                if c >= h.n:
                    assert prefix(*h.range[c]) > prefix(f, l)


def test_keys_definition():
    """Cells and codes on inputs whose answer is known: the corners of the centroid box, an axis without extent, x in the highest bit."""
    tri = lambda c: np.float32([c, c, c])
    P = np.stack([tri([0, 0, 0]), tri([1, 2, 4]), tri([1, 0, 0]), tri([0, 2, 0]), tri([0, 0, 4]), tri([0.5, 1, 2])])
    q = br.cells(P)
    assert q.tolist() == [[0, 0, 0], [1023, 1023, 1023], [1023, 0, 0], [0, 1023, 0], [0, 0, 1023], [512, 512, 512]]
    keys = br.morton_keys(P)
    code = [k >> 32 for k in keys]
    assert [k & 0xffffffff for k in keys] == list(range(6))
    assert code[0] == 0 and code[1] == (1 << 30) - 1
    assert code[2] == 0b100100100100100100100100100100 and code[3] == code[2] >> 1 and code[4] == code[2] >> 2
    assert code[5] == 0b111 << 27
    flat = P.copy()
    flat[:, :, 1] = 7.0  # no extent on y: every y cell is 0
    assert (br.cells(flat)[:, 1] == 0).all()
    one = br.positions_of(br.host_export(br.scene_cases(4)["one_centroid"], 4))
    assert (br.cells(one) == 0).all() and one.shape[0] == 300, "the case with one common centroid has every code 0"
    z = br.centroids(positions("zeros"))
    assert np.signbit(z[z[:, 0] == 0, 0]).any() and not np.signbit(z[z[:, 0] == 0, 0]).all(), "the zeros case has centroids at -0.0 and at +0.0"


@pytest.mark.parametrize("name", SMALL + ("grid_x3",))
def test_lbvh_reference_equals_karras(name):
    """The recursive definition and Karras' per-node search give one tree: same canonical form at every leaf size."""
    for leaf in br.LEAF_SIZES:
        P = positions(name, leaf)
        a, b = br.lbvh_hierarchy(P), br.karras_hierarchy(P)
        pad = br.scene_pad(P)
        for ls in br.LEAF_SIZES:
            ta, tb = br.layout(a, ls, pad), br.layout(b, ls, pad)
            assert ta.form == tb.form and (ta.depth, ta.max_leaf) == (tb.depth, tb.max_leaf)
        assert sorted(a.range.values()) == sorted(b.range.values())


def plain_nearest(lo, hi, radius):
    """For every cluster the first j != i within `radius` positions (None: any) with the smallest union area: a plain double loop."""
    m = len(lo)
    out = []
    for i in range(m):
        best, bj = F32(np.inf), -1
        for j in range(0 if radius is None else max(0, i - radius), m if radius is None else min(m - 1, i + radius) + 1):
            if j == i:
                continue
            d = np.maximum(hi[i], hi[j]) - np.minimum(lo[i], lo[j])
            a = F32(F32(F32(d[0] * d[1]) + F32(d[1] * d[2])) + F32(d[2] * d[0]))
            if a < best:
                best, bj = a, j
        out.append(bj)
    return out


@pytest.mark.parametrize("name", SMALL)
def test_ploc_reference_rounds(name):
    P = positions(name)
    n = P.shape[0]
    # (the unbounded double loop is quadratic per round: on the cases of up to 130 triangles)
    for radius, plain_radius in ((1, 1), (br.DEFAULT_RADIUS, br.DEFAULT_RADIUS)) + (((n, None), (4 * n + 5, None)) if n <= 130 else ()):
        trace = []
        h = br.ploc_hierarchy(P, radius, trace)
        assert h.rounds == len(trace) and len(h.left) == 2 * n - 1 and h.count[h.root] == n
        for cid, nn, low in trace:
            want = plain_nearest([h.lo[c] for c in cid], [h.hi[c] for c in cid], plain_radius)
            assert nn.tolist() == want
            mutual = [i for i in range(len(cid)) if want[i] >= 0 and want[want[i]] == i]
            assert sorted(low.tolist() + [want[i] for i in low]) == mutual, "merged pairs are exactly the mutual ones"
            assert all(i < want[i] for i in low)
        for leaf in br.LEAF_SIZES:
            check_layout(P, br.layout(h, leaf, br.scene_pad(P)))
        assert br.ploc_rounds(P, radius) == h.rounds
    big, unbounded = br.ploc_hierarchy(P, n), br.ploc_hierarchy(P, 4 * n + 5)
    assert br.layout(big, 1, F32(0)).form == br.layout(unbounded, 1, F32(0)).form


def test_ploc_merge_order():
    """Children are (lower position, higher position), the node takes the lower position, the rest keep their place: four triangles in
    a row whose middle two are closest."""
    x = np.float32([0.0, 4.0, 5.0, 9.5])
    P = np.stack([np.stack([[v, 0, 0], [v + 0.5, 0, 0], [v, 0.5, 0]]) for v in x]).astype(np.float32)
    h = br.ploc_hierarchy(P, 16)
    assert h.order == [0, 1, 2, 3] and h.rounds == 3
    assert (h.left[4], h.right[4]) == (1, 2) and (h.left[5], h.right[5]) == (0, 4) and (h.left[6], h.right[6]) == (5, 3) and h.root == 6
    assert br.layout(h, 1, F32(0)).depth == 3 and [e[1] for e in br.layout(h, 2, F32(0)).form if e[0] == "L"] == [(0,), (1, 2), (3,)]


@pytest.mark.parametrize("name", br.CASE_NAMES)
def test_host_only_context_holds_builder0(name):
    for leaf in br.LEAF_SIZES:
        tris = br.scene_cases(leaf)[name]
        want = br.export_bytes(br.host_export(tris, leaf, 0))
        for builder in (1, 2):
            assert br.export_bytes(br.host_export(tris, leaf, builder, radius=br.DEFAULT_RADIUS)) == want, (leaf, builder)


def test_case_table():
    """What the GPU tests expect of every case, from the references alone."""
    table, t0 = {}, time.time()
    for name in br.CASE_NAMES:
        for builder in (1, 2):
            for leaf, radius in br.combos(builder):
                P = positions(name, leaf)
                if P.shape[0] <= leaf:  # stays on the host (test 5 of the GPU file): nothing to expect of a device tree
                    assert name in ("n2", "n3") and leaf > 1
                    continue
                ref, h = br.reference(P, builder, leaf, radius)
                row = dict(triangles=int(P.shape[0]), depth=ref.depth, nodes=ref.n_nodes, max_leaf=ref.max_leaf)
                if builder == 2:
                    row["rounds"] = h.rounds
                    assert h.rounds <= br.PLOC_ROUND_CAP
                assert not ref.too_deep(br.DEFAULT_MAX_DEPTH, builder) and ref.depth <= 48, (name, builder, leaf, radius, ref.depth)
                assert ref.n_nodes >= 1 and ref.max_leaf <= leaf
                table["%s/builder%d/leaf%d/radius%d" % (name, builder, leaf, radius if builder == 2 else 0)] = row
    # n = 2 and 3 reach the device at leaf size 1, n = leaf_size + 1 always
    assert all("%s/builder%d/leaf1/radius%d" % (n, b, r) in table for n in ("n2", "n3") for b, r in ((1, 0), (2, 16)))
    # test 3: the Cornell box under max_bvh_depth = 14 - both device trees are deeper, the host builder keeps to the limit
    P = positions("cornell")
    fallback = {}
    for builder in (1, 2):
        ref, _ = br.reference(P, builder, 4)
        assert ref.too_deep(br.FALLBACK_DEPTH, builder) and ref.depth > br.FALLBACK_DEPTH
        fallback["builder%d" % builder] = ref.depth
    assert br.host_export(br.scene_cases(4)["cornell"], 4, 0, max_depth=br.FALLBACK_DEPTH)["depth"] <= br.FALLBACK_DEPTH
    br.write_profile("reference", dict(cases=table, cornell_depth_against_max_bvh_depth_14=fallback, seconds=round(time.time() - t0, 1)))


def test_round_cap_strips():
    """Test 4 of the GPU file.  ray_battery.strip_scene(9000) stays below the cap in the reference (its round count levels off:
    builder_ref.level_strip), so a device tree is expected there, and it is the reference's; the level strip of the same length lies
    beyond the cap, so the host builder is expected to take over.  The figures the GPU test reads from tests/golden are those computed
    here."""
    gold = br.golden_rounds()
    P = br.positions_of(br.host_export(rb.strip_scene(600), 4))
    assert br.ploc_rounds(P) == gold["strip_scene_600"]["rounds"]
    P = br.positions_of(br.host_export(rb.strip_scene(br.STRIP_N), 4))
    h = br.ploc_hierarchy(P, br.DEFAULT_RADIUS)
    ref = br.layout(h, 4, br.scene_pad(P))
    g = gold["strip_scene_%d" % br.STRIP_N]
    assert (h.rounds, ref.depth, ref.n_nodes) == (g["rounds"], g["depth"], g["nodes"])
    assert br.form_digest(ref.form, ref.pad, ref.depth, ref.max_leaf) == g["digest"]
    assert h.rounds <= br.PLOC_ROUND_CAP and not ref.too_deep(br.DEFAULT_MAX_DEPTH, 2), "a device tree is expected"
    P = br.positions_of(br.host_export(br.level_strip(br.STRIP_N), 4))
    rounds = br.ploc_rounds(P)
    assert rounds == gold["level_strip_%d" % br.STRIP_N]["rounds"] and rounds > br.PLOC_ROUND_CAP, "a fallback is expected"
    br.write_profile("round_cap_reference", {k: v for k, v in gold.items()})
