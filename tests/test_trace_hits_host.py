"""pt_trace_hits without a GPU (include/mi355pt.h "ray queries: the first K hits"): the CPU twin pt_debug_trace_hits_host against the
oracle-derived rule of tests/hits_ref.py, bit for bit.

* The four exports exist, are in B.EXPORTS and in the header; pt_hits_params is 16 bytes with the defaults {4, 0, 0, 0}; the ABI version
  is still 5; the _device form is in both lists of the streams contract and the blocking form in the list of blocking calls.
* The rule rejects deliberately wrong lists (a dropped tie partner, swapped entries, a dropped hit at exactly thi, a kept hit below 1e-3)
  and accepts the right ones they were made from.
* The twin against the rule on every scene of the ray battery and on the constructed stacks, K = 1, 2, 3, 4, 16, on ALL compared rays;
  K = 1 against pt_debug_trace_rays_host on every ray; the list for K is the prefix of the list for 16 on every ray.
* The doubled stack against its lists by construction: both partners of every tie, the lower id first, a tie at exactly thi included.
* The bounds tmax = t of a hit, nextafter(t, 0), NaN, +inf, -1, 1e-3.
* "watertight" 0 and 1 on the closed icosphere: entry 0 is the oracle's answer; after pt_update_vertices the twin equals a fresh upload's.
* Every refusal by name and the host-only return codes; n = 0; `make asm-rays-hits`: four instances, no scratch, at most 128 VGPRs."""
import ctypes as C
import re

import numpy as np
import pytest

import hits_common as HC
import hits_ref
import ray_battery as rb
import resource_report
import trace_rays_common as TC
from owl_path_tracer_amd.pyhost import binding as B

PT_E_INVALID, PT_E_NO_DEVICE, PT_E_NO_SCENE = -1, -2, -4
NAMES = ("pt_hits_default_params", "pt_trace_hits", "pt_trace_hits_device", "pt_debug_trace_hits_host")


def _host(tris, **opts):
    ctx = B.Context(-1)
    for k, v in opts.items():
        ctx.set_option(k, v)
    rb.upload(ctx, tris)
    return ctx


def test_exports_abi_and_records():
    L = B.lib()
    header = open(B.HEADER_PATH).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in B.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.pt_abi_version() == 5 and re.search(r"#define PT_ABI_VERSION 5\b", header)
    assert re.search(r"#define PT_HITS_MAX 16\b", header) and B.PT_HITS_MAX == 16 and C.sizeof(B.HitsParams) == 16
    p = B.HitsParams(9, (9, 9, 9))
    L.pt_hits_default_params(C.byref(p))
    assert (p.max_hits, list(p.reserved)) == (4, [0, 0, 0])
    L.pt_hits_default_params(None)
    assert "pt_trace_hits_device" in re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)
    assert "pt_trace_hits_device" in re.search(r"Waits on the host for the context's last asynchronous call - (.*?) - and for the context's own stream", header, flags=re.S).group(1)
    assert re.search(r"The blocking renders \([^)]*\),[^\n]*\bpt_trace_hits\b", header)
    assert "NOT BUILT: a per-ray lower bound or (t, id) floor" in header


def test_the_rule_rejects_wrong_lists(orc):
    c = HC.case(orc, "stack_doubled")
    ctx = _host(c["tris"])
    l16, l4 = ctx.trace_hits_host(c["rec"], 16), ctx.trace_hits_host(c["rec"], 4)
    ctx.close()
    b = c["bounds"]
    # ray 0: straight through 20 quads, 30 triangles: its list of 16 is full, entries 1 and 2 are the first doubled quad;
    # ray b: tmax exactly the t of the third quad: four hits with K = 16 ... and with K = 4 no room, so K = 16 is used; ray 1 is tilted
    assert l16["prim"][0, -1] >= 0 and l16["t"][0, 1] == l16["t"][0, 2] and c["length"][0] == hits_ref.LEVELS
    at_thi = l16[b]
    assert at_thi["t"][3] == c["rec"]["tmax"][b] and at_thi["prim"][4] < 0
    short = np.nonzero((l4["prim"][:, 0] >= 0) & (l4["prim"][:, -1] < 0))[0]
    assert short.size, "a tilted ray leaves the stack after fewer than four triangles"
    rows = [0, b, int(short[0])]
    right = [l16[0], at_thi, l4[short[0]]]
    for lst, i in zip(right, rows):
        assert not hits_ref.check_lists(lst[None], c["chain"][i:i + 1], c["length"][i:i + 1], c["rec"][i:i + 1], c["real"]), "a right list is rejected"
    muts = hits_ref.mutations((l16[0], 2), at_thi, l4[short[0]])
    assert len(muts) >= 4
    for label, slot, lst in muts:
        i = rows[slot]
        bad = hits_ref.check_lists(lst[None], c["chain"][i:i + 1], c["length"][i:i + 1], c["rec"][i:i + 1], c["real"])
        print("%-40s rejected: %s" % (label, bad[0][1] if bad else "NO"))
        assert bad, "the rule accepts a wrong list: " + label
    # a second partner that is no triangle of the scene at that t is not REAL
    fake = l16[0].copy()
    fake["prim"][2] = fake["prim"][1] + 1  # the quad's other triangle, which the ray does not cross
    assert hits_ref.check_lists(fake[None], c["chain"][:1], c["length"][:1], c["rec"][:1], c["real"])


@pytest.mark.parametrize("name", HC.names())
def test_twin_against_the_rule(orc, name):
    c = HC.case(orc, name)
    rec = c["rec"]
    ctx = _host(c["tris"])
    lists = {K: ctx.trace_hits_host(rec, K) for K in HC.KS}
    closest = ctx.trace_rays_host(rec)
    ctx.close()
    print("%s: %d rays, %d compared, chain levels: mean %.2f, %d rays with >= 2, %d with >= 16" % (
        name, rec.shape[0], c["idx"].size, c["length"].mean(), (c["length"] >= 2).sum(), (c["length"] >= 16).sum()))
    for K in HC.KS:
        assert lists[K].shape == (rec.shape[0], K)
        HC.assert_rule(c, lists[K], "%s, K = %d: twin vs the rule" % (name, K))
        HC.assert_same_lists(lists[K], lists[16][:, :K], None, "%s: the list for K = %d is the prefix of the list for 16" % (name, K), rec)
    assert TC.same(np.ascontiguousarray(lists[1][:, 0]), closest).all(), "K = 1 is pt_debug_trace_rays_host, on every ray"
    assert TC.same(np.ascontiguousarray(lists[16][:, 0]), closest).all(), "entry 0 is the closest hit, on every ray"


def test_the_cases_do_not_go_empty(orc):
    """Some compared ray has a full list of 16, some list has a tie, and the battery has rays with several levels."""
    c = HC.case(orc, "stack_doubled")
    ctx = _host(c["tris"])
    l16 = ctx.trace_hits_host(c["rec"], 16)
    ctx.close()
    assert (l16["prim"][c["mask"], -1] >= 0).any(), "no full list of 16"
    tie = (l16["t"][:, 1:] == l16["t"][:, :-1]) & (l16["prim"][:, 1:] >= 0)
    assert tie.any() and (tie.sum(1) >= 5).any(), "no list with ties"
    plain = HC.case(orc, "stack")
    assert (plain["length"] == hits_ref.LEVELS).any() and ((plain["length"] > 0) & (plain["length"] < 16)).any()
    for name in ("rects", "cornell", "dragon", "car"):
        assert (HC.case(orc, name)["length"] >= 2).sum() >= 500, name
    r = HC.case(orc, "rects")
    ctx = _host(r["tris"])
    l4 = ctx.trace_hits_host(r["rec"], 4)[r["mask"]]
    ctx.close()
    assert ((l4["t"][:, 1:] == l4["t"][:, :-1]) & (l4["prim"][:, 1:] >= 0)).any(), "the coincident copies of rects give ties on battery rays"


@pytest.mark.parametrize("K", HC.KS)
def test_doubled_stack_by_construction(orc, K):
    c = HC.case(orc, "stack_doubled")
    ctx = _host(c["tris"])
    got = ctx.trace_hits_host(c["rec"], K)
    ctx.close()
    HC.assert_same_lists(got, HC.doubled_expectation(c, K), None, "stack_doubled, K = %d: the lists by construction" % K, c["rec"])


def test_bounds(orc):
    for name in HC.CONSTRUCTED:
        c = HC.case(orc, name)
        b = c["bounds"]
        ctx = _host(c["tris"])
        got = ctx.trace_hits_host(c["rec"], 16)
        ctx.close()
        n = (got["prim"] >= 0).sum(1)
        per_quad = 1.5 if name == "stack_doubled" else 1.0  # triangles crossed per quad, on average over an original and a doubled one
        assert n[b] == int(2 * per_quad) + 1 and got["t"][b, n[b] - 1] == c["rec"]["tmax"][b], "tmax = t of the third quad: kept"
        assert n[b + 1] == n[b] - 1, "nextafter(t, 0): gone"
        assert HC.same_lists(got[b + 2:b + 4], got[[0, 0]]).all(), "NaN and +inf: the library's bound"
        assert (n[b + 4:b + 6] == 0).all(), "tmax -1 and 1e-3: the interval is empty"
        assert n[b + 6] == (3 if name == "stack_doubled" else 2) and (got["t"][b + 6, n[b + 6] - 1] == c["rec"]["tmax"][b + 6])


def test_closed_mesh_both_tests(orc):
    tris, rays, mt, wt = TC.closed_case(orc)
    assert wt[0].all()
    ctx = _host(tris, watertight=1)
    got = ctx.trace_hits_host(rays, 4)
    TC.assert_same(np.ascontiguousarray(got[:, 0]), TC.hits_of(wt), None, "closed mesh, watertight: entry 0", rays)
    assert TC.same(ctx.trace_hits_host(rays, 1).reshape(-1), TC.hits_of(wt)).all()
    ctx.set_option("watertight", 0)
    TC.assert_same(np.ascontiguousarray(ctx.trace_hits_host(rays, 4)[:, 0]), TC.hits_of(mt), None, "closed mesh, Moeller-Trumbore: entry 0", rays)
    ctx.close()


def test_after_update_vertices(orc):
    tris, moved = TC.moved_scene()
    rec = HC.case(orc, "soup1")["rec"]
    ctx = _host(tris, dynamic=1)
    before = ctx.trace_hits_host(rec, 4)
    ctx.update_vertices([rb.mesh_of(moved)])
    fresh = _host(moved)
    want = fresh.trace_hits_host(rec, 4)
    assert not HC.same_lists(want, before).all(), "the deformation changes lists"
    HC.assert_same_lists(ctx.trace_hits_host(rec, 4), want, None, "twin after pt_update_vertices vs a fresh upload", rec)
    ctx.close()
    fresh.close()


def test_refusals_and_error_codes():
    L = B.lib()
    vp = C.c_void_p
    rays = B.make_rays(np.float32([[0.1, 0.1, 3.0, 0, 0, -1]] * 4))
    out = np.full(4 * 16 * 4, 7, np.int32)
    r, o = rays.ctypes.data_as(vp), out.ctypes.data_as(vp)
    v16 = vp(16)
    ctx = B.Context(-1)
    hd = ctx._h
    ok, none = C.byref(B.hits_params(16)), None
    block = lambda rr, n, p, oo: L.pt_trace_hits(hd, rr, n, p, oo)
    dev = lambda rr, n, p, oo: L.pt_trace_hits_device(hd, rr, n, p, oo, None)
    twin = lambda rr, n, p, oo: L.pt_debug_trace_hits_host(hd, rr, n, p, oo)
    forms = ((block, "pt_trace_hits", r, o, "rays", "out"), (dev, "pt_trace_hits_device", v16, v16, "d_rays", "d_out"), (twin, "pt_debug_trace_hits_host", r, o, "rays", "out"))

    def msg():
        return L.pt_last_error(hd).decode()

    for fn, who, rr, oo, _, _ in forms:
        assert fn(rr, 4, ok, oo) == PT_E_NO_SCENE and who in msg()
    rb.upload(ctx, rb.make_scene("rects"))
    for fn, who, rr, oo, nr, no in forms:
        for k in (0, -1, 17, 2 ** 31 - 1):
            assert fn(rr, 4, C.byref(B.hits_params(k)), oo) == PT_E_INVALID and who + ": max_hits %d outside 1..16" % k in msg()
        for w in range(3):
            p = B.hits_params(4)
            p.reserved[w] = 1
            assert fn(rr, 4, C.byref(p), oo) == PT_E_INVALID and who in msg() and "reserved" in msg()
        for p in (ok, none):
            assert fn(None, 4, p, oo) == PT_E_INVALID and who + ": NULL " + nr in msg()
            assert fn(rr, 4, p, None) == PT_E_INVALID and who + ": NULL " + no in msg()
            for n in (-1, 2 ** 31):
                assert fn(rr, n, p, oo) == PT_E_INVALID and who + ": n = %d" % n in msg()
    assert L.pt_trace_hits(None, r, 4, ok, o) == PT_E_INVALID and L.pt_trace_hits_device(None, v16, 4, ok, v16, None) == PT_E_INVALID
    assert L.pt_debug_trace_hits_host(None, r, 4, ok, o) == PT_E_INVALID
    for bad in (vp(24), vp(4), vp(17)):
        assert dev(bad, 4, ok, v16) == PT_E_INVALID and "pt_trace_hits_device: d_rays is not 16-byte aligned" in msg()
        assert dev(v16, 4, ok, bad) == PT_E_INVALID and "pt_trace_hits_device: d_out is not 16-byte aligned" in msg()
    # a host-only context: valid arguments give PT_E_NO_DEVICE (n = 0 included), and the twin works
    for p in (ok, none):
        assert block(r, 4, p, o) == PT_E_NO_DEVICE and dev(v16, 4, p, v16) == PT_E_NO_DEVICE
        assert block(None, 0, p, None) == PT_E_NO_DEVICE and dev(None, 0, p, None) == PT_E_NO_DEVICE
    assert (out == 7).all(), "a refused call wrote to the output"
    ctx.set_option("quad", 0)  # the device forms need quad nodes: refused by name, invalid arguments first; the twin walks the binary tree
    assert block(r, 4, ok, o) == PT_E_INVALID and "pt_trace_hits" in msg() and "quad" in msg()
    assert dev(v16, 4, ok, v16) == PT_E_INVALID and "pt_trace_hits_device" in msg() and "quad" in msg()
    assert block(None, 4, ok, o) == PT_E_INVALID and "NULL rays" in msg()
    assert twin(r, 4, none, o) == 4  # NULL parameters: the defaults, K = 4
    got = out.view(B.HIT_DTYPE)
    assert (got["prim"][:16] >= 0).any() and (out[64:] == 7).all(), "the twin writes n * K records and nothing behind them"
    assert twin(r, 4, ok, o) == 4 and (out.view(B.HIT_DTYPE)["prim"].reshape(4, 16)[:, 0] >= 0).all()
    ctx.close()


def test_n_zero():
    ctx = _host(rb.make_scene("one_leaf"))
    none = np.zeros(0, B.RAY_DTYPE)
    assert ctx.trace_hits_host(none, 16).shape == (0, 16)
    assert B.lib().pt_debug_trace_hits_host(ctx._h, None, 0, None, None) == 0
    ctx.close()


def test_hits_kernels_resources():
    """From the Makefile's own target (the flags that ship): the two EXACT instances of each translation unit and nothing else, no scratch,
    at most 128 VGPRs."""
    blocks = resource_report.report("asm-rays-hits")[1]
    names = [b[0] for b in blocks]
    assert len(blocks) == 4 and len(set(names)) == 4, names
    assert sum("pt_rays_hits_wt_kernel" in nm for nm in names) == 2 and sum("pt_rays_hits_kernel" in nm for nm in names) == 2, names
    for nm, vgprs, scratch in blocks:
        assert int(scratch) == 0 and 0 < int(vgprs) <= 128, (nm, vgprs, scratch)
