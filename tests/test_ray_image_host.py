"""Ray images (pt_render_rays; include/mi355pt.h "ray images") without a GPU.

* The two exports exist, are in B.EXPORTS and in the header, the record is 64 bytes with the fields where the header puts them, the ABI
  version is still 5 and the _device form is in both lists of the streams contract.
* Every refusal of the header on a host-only context, by code and by message; a refused call writes nothing.  (A communicator needs a
  device: that refusal is tests/test_gpu_ray_image.py's.)
* pyhost/ray_image.py: pinhole against gen_camera_ray's formula in float64, equirect against its formula, fixed and to_list.
* tests/ray_image_ref.py itself: through a degenerate camera the oracle's pixel depends on the pixel's stream on a diffuse wall and not on
  sky, and the 1 x 1 form is the camera it names.
* The oracle's ray-image generator (Scene.render_rays), anchored before the GPU tests hold anything to it: with zero jitter it is the
  degenerate camera bit for bit (frame, RGBA8, counters; 1 and many threads; a pixel list); eight jittered 1 x 1 records are the camera
  they name; on a table with per-pixel jitter the first ray of samples 0 to 7 of every pixel is the numpy restatement's; the
  reserved floats are not read; a restatement that takes the neighbouring record's du / dv, swaps rx and ry or adds dv before du is told
  apart, ray by ray and as a 1 spp frame; and the tables of tests/ray_tables.py meet their precondition at every size and sample count
  the GPU tests use.
* `make asm-rayimage`: exactly the five instances, no scratch, the 4-wave instances within 128 VGPRs."""
import ctypes as C
import re

import numpy as np
import pytest

import aov_common as AC
import aov_rays_ref
import ray_image_ref as RR
import ray_tables as RT
import resource_report
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import ray_image as RI

F32 = np.float32
PT_E_INVALID, PT_E_NO_DEVICE, PT_E_NO_SCENE = -1, -2, -4
NAMES = ("pt_render_rays", "pt_render_rays_device")


def test_exports_abi_and_record():
    L = B.lib()
    header = open(B.HEADER_PATH).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in B.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.pt_abi_version() == 5 and re.search(r"#define PT_ABI_VERSION 5\b", header)
    assert "pt_render_rays_device" in re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)
    assert "pt_render_rays_device" in re.search(r"Waits on the host for the context's last asynchronous call - (.*?) - and for the context's own stream", header, flags=re.S).group(1)
    # sizeof(pt_ray_gen) == 64: the struct as the header declares it, laid out by ctypes with the C rules
    body = re.search(r"typedef struct pt_ray_gen \{(.*?)\} pt_ray_gen;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"float\s+(\w+)(?:\[(\d+)\])?\s*;", body)
    assert [f for f, _ in fields] == ["org", "reserved0", "dir", "reserved1", "du", "reserved2", "dv", "reserved3"]

    class RayGen(C.Structure):
        _fields_ = [(f, C.c_float * int(n) if n else C.c_float) for f, n in fields]

    assert C.sizeof(RayGen) == 64 and B.RAY_GEN_DTYPE.itemsize == 64 and RI.DTYPE is B.RAY_GEN_DTYPE
    for f, _ in fields:
        assert B.RAY_GEN_DTYPE.fields[f][1] == getattr(RayGen, f).offset, f
    assert [B.RAY_GEN_DTYPE.fields[k][1] for k in ("org", "dir", "du", "dv")] == [0, 16, 32, 48]


def _cornell_host():
    ctx = B.Context(-1)
    AC.upload(ctx, AC.scene("cornell"), B)
    return ctx


def test_refusals_and_error_codes():
    L = B.lib()
    vp = C.c_void_p
    W, H = 5, 3
    rays = RI.fixed((0.0, 1.0, 3.0), (0.0, 0.0, -1.0), W, H)
    rgb = np.full((H, W, 3), 7.0, F32)
    rgba = np.full((H, W), 7, np.uint32)
    r, o, o8 = rays.ctypes.data_as(vp), rgb.ctypes.data_as(C.POINTER(C.c_float)), rgba.ctypes.data_as(C.POINTER(C.c_uint32))
    v16 = vp(16)
    ctx = B.Context(-1)
    hd = ctx._h

    def msg():
        return L.pt_last_error(hd).decode()

    def blocking(rr=r, w=W, h=H, spp=4, depth=8, out=o):
        return L.pt_render_rays(hd, rr, w, h, spp, depth, out, o8)

    def device(rr=v16, w=W, h=H, spp=4, depth=8, out=v16):
        return L.pt_render_rays_device(hd, rr, w, h, spp, depth, out, None, None)

    forms = ((blocking, "pt_render_rays", "rays", "out_rgb"), (device, "pt_render_rays_device", "d_rays", "d_out_rgb"))
    # without a scene
    for fn, who, _, _ in forms:
        assert fn() == PT_E_NO_SCENE and "pt_upload_scene not called" in msg()
    AC.upload(ctx, AC.scene("cornell"), B)
    assert L.pt_render_rays(None, r, W, H, 4, 8, o, o8) == PT_E_INVALID
    assert L.pt_render_rays_device(None, v16, W, H, 4, 8, v16, None, None) == PT_E_INVALID
    for fn, who, rname, oname in forms:
        assert fn(rr=None) == PT_E_INVALID and "%s: NULL %s" % (who, rname) in msg()
        assert fn(out=None) == PT_E_INVALID and "%s: NULL %s" % (who, oname) in msg()
        # the sizes and depths pt_render refuses
        for kw in (dict(w=0), dict(h=0), dict(w=-1), dict(w=65536), dict(h=65536), dict(spp=0), dict(spp=-3), dict(depth=-1), dict(depth=64)):
            assert fn(**kw) == PT_E_INVALID and "bad render size" in msg(), kw
        # options that only exist for a camera's frame
        for key, value, default, word in (("watertight", 1, 0, "watertight"), ("kernel", 1, 2, "kernel = 1"), ("latency", 1, 0, "latency"), ("timeline", 1, 0, "timeline")):
            ctx.set_option(key, value)
            try:
                assert fn() == PT_E_INVALID and who + ":" in msg() and word in msg(), (key, msg())
                assert fn(rr=None) == PT_E_INVALID and "NULL" in msg()  # invalid arguments first
            finally:
                ctx.set_option(key, default)
        assert fn() == PT_E_NO_DEVICE  # valid arguments: no CPU fallback behind the entry point
    for bad in (vp(24), vp(4), vp(17), vp(72)):
        assert device(rr=bad) == PT_E_INVALID and "pt_render_rays_device: d_rays is not 16-byte aligned" in msg()
    assert device(rr=vp(64), out=vp(4)) == PT_E_NO_DEVICE  # the frame is floats: any float address
    # the records, which the blocking form reads: not finite, or no direction
    for field in ("org", "dir", "du", "dv"):
        for bad in (np.nan, np.inf, -np.inf):
            for i, comp in ((0, 0), (7, 1), (W * H - 1, 2)):
                t = rays.copy()
                t[field][i, comp] = bad
                assert L.pt_render_rays(hd, t.ctypes.data_as(vp), W, H, 4, 8, o, o8) == PT_E_INVALID
                assert "pt_render_rays: record %d (pixel %d, %d): %s is not finite" % (i, i % W, i // W, field) in msg(), msg()
    t = rays.copy()
    t["dir"][9] = (0.0, -0.0, 0.0)
    assert L.pt_render_rays(hd, t.ctypes.data_as(vp), W, H, 4, 8, o, o8) == PT_E_INVALID and "record 9 (pixel 4, 1): dir is 0" in msg()
    t = rays.copy()  # the reserved floats are not read: anything may stand there; a zero jitter and a tiny direction are rays
    for k in range(4):
        t["reserved%d" % k] = np.nan
    t["dir"][3] = (0.0, 1e-30, 0.0)
    assert L.pt_render_rays(hd, t.ctypes.data_as(vp), W, H, 4, 8, o, o8) == PT_E_NO_DEVICE
    assert (rgb == 7.0).all() and (rgba == 7).all(), "a refused call wrote to its outputs"
    with pytest.raises(B.PtError, match="records for a 5x3 ray image"):
        ctx.render_rays(rays[:-1], W, H, 4, 8)
    with pytest.raises(B.PtError, match="no CPU fallback"):
        ctx.render_rays(rays, W, H, 4, 8)
    ctx.close()


def test_pinhole_against_the_camera_formula():
    """pinhole's record holds three float32 vectors, each the float64 value rounded once: dir = llc + hor * x / W + ver * y / H - origin,
    du = hor / W, dv = ver / H.  Evaluated in float64, dir + du * rx + dv * ry therefore differs from gen_camera_ray's unnormalised
    direction llc + hor * (x + rx) / W + ver * (y + ry) / H - origin (float64, from the same float32 camera) by at most the three roundings
        ulp(dir) / 2 + rx * ulp(du) / 2 + ry * ulp(dv) / 2  <=  3 * 2^-24 * M        (rx, ry < 1, ulp(v) <= 2^-23 |v|)
    per component, M the largest magnitude among the components of dir, du and dv: 1.5 float32 ulps of the largest term.  The float64
    evaluations themselves add some 1e-16 * M, which 1e-12 * M covers."""
    for name, W, H in (("cornell", 20, 13), ("cube", 64, 48), ("ico_map", 7, 5)):
        cam = AC.camera(AC.scene(name), W, H, B.to_camera_data)
        a = cam.as_array().astype(np.float64)
        o, llc, hor, ver = a[0:3], a[3:6], a[6:9], a[9:12]
        t = RI.pinhole(cam, W, H)
        assert t.shape == (W * H,) and t.dtype == B.RAY_GEN_DTYPE
        assert (t["org"] == cam.as_array()[0:3]).all()
        x = np.tile(np.arange(W), H)[:, None].astype(np.float64)
        y = np.repeat(np.arange(H), W)[:, None].astype(np.float64)
        d, du, dv = (t[k].astype(np.float64) for k in ("dir", "du", "dv"))
        M = max(np.abs(d).max(), np.abs(du).max(), np.abs(dv).max())
        bound = 3.0 * 2.0 ** -24 * M + 1e-12 * M
        worst = 0.0
        for rx in (0.0, 0.5):
            for ry in (0.0, 0.5):
                want = llc + hor * ((x + rx) / W) + ver * ((y + ry) / H) - o
                got = d + du * rx + dv * ry
                worst = max(worst, np.abs(got - want).max())
        print("%s %dx%d: largest term %.4g, worst direction error %.3g (%.2f ulp of it), bound %.3g" % (name, W, H, M, worst, worst / (2.0 ** -23 * M), bound))
        assert worst <= bound
        for k in range(4):
            assert (t["reserved%d" % k] == 0).all()
    assert (RI.pinhole(cam.as_array(), 7, 5).tobytes() == t.tobytes())  # the 12 floats do as well as the Camera


def test_equirect_against_its_formula():
    W, H = 16, 8
    origin = (0.25, 1.0, -0.5)
    t = RI.equirect(origin, W, H)
    assert t.shape == (W * H,) and (t["org"] == F32(origin)).all()
    d, du, dv = (t[k].astype(np.float64) for k in ("dir", "du", "dv"))
    centre = d + 0.5 * du + 0.5 * dv
    # unit length: three float32 roundings of values below 1 (see test_pinhole_against_the_camera_formula) on a unit vector
    assert np.abs(np.linalg.norm(centre, axis=1) - 1.0).max() <= 3 * 3.0 * 2.0 ** -24
    for x, y in ((0, 0), (W // 2, H // 2), (W - 1, H - 1), (3, 6), (W // 4, H // 2 - 1)):
        phi = 2 * np.pi * ((x + 0.5) / W - 0.5)
        th = np.pi * ((y + 0.5) / H - 0.5)
        # forward = -z, up = +y, right = forward x up = +x
        want = np.array([np.cos(th) * np.sin(phi), np.sin(th), -np.cos(th) * np.cos(phi)])
        assert np.abs(centre[x + W * y] - want).max() <= 3 * 2.0 ** -24 + 1e-12, (x, y)
    # where the formula says in words: the middle of the image looks forward, rows go up, columns go right, the seam is behind
    mid = centre[W // 2 + W * (H // 2)]
    assert mid[2] < -0.9 and centre[W // 2 + W * (H - 1)][1] > 0.9 and centre[W // 2 + W * 0][1] < -0.9
    assert centre[3 * W // 4 + W * (H // 2)][0] > 0.9 and centre[W // 4 + W * (H // 2)][0] < -0.9 and centre[0 + W * (H // 2)][2] > 0.9
    # du, dv: the finite differences to the neighbouring pixel's centre
    for x, y in ((2, 3), (W - 1, 1), (5, H - 1)):
        c0 = RI.equirect_direction(x + 0.5, y + 0.5, W, H)
        assert np.abs(du[x + W * y] - (RI.equirect_direction(x + 1.5, y + 0.5, W, H) - c0)).max() <= 2.0 ** -23
        assert np.abs(dv[x + W * y] - (RI.equirect_direction(x + 0.5, y + 1.5, W, H) - c0)).max() <= 2.0 ** -23
    # another frame: forward +x, up +z
    t2 = RI.equirect(origin, W, H, up=(0, 0, 2), forward=(3, 0, 0))
    c2 = (t2["dir"].astype(np.float64) + 0.5 * t2["du"] + 0.5 * t2["dv"])
    assert c2[W // 2 + W * (H // 2)][0] > 0.9 and c2[W // 2 + W * (H - 1)][2] > 0.9
    with pytest.raises(ValueError, match="parallel"):
        RI.equirect(origin, W, H, up=(0, 0, -1))


def test_fixed_and_to_list():
    W, H = 4, 3
    orgs = np.arange(W * H * 3, dtype=F32).reshape(-1, 3)
    dirs = -orgs - 1
    t = RI.fixed(orgs, dirs, W, H)
    assert (t["org"] == orgs).all() and (t["dir"] == dirs).all() and (t["du"] == 0).all() and (t["dv"] == 0).all()
    assert np.ascontiguousarray(t).view(np.uint32).reshape(-1, 16)[:, [3, 7, 11, 15]].max() == 0
    assert (RI.fixed((1, 2, 3), dirs, W, H)["org"] == F32([1, 2, 3])).all()
    with pytest.raises(ValueError):
        RI.fixed(orgs[:-1], dirs, W, H)
    # a frame in framebuffer order whose pixel (x, y) holds its launch index
    frame = np.zeros((H, W, 3), F32)
    for y in range(H):
        for x in range(W):
            frame[H - 1 - y, x] = x + W * y
    assert (RI.to_list(frame, W, H) == np.arange(W * H, dtype=F32)[:, None]).all()
    assert (RI.to_list(frame[..., 0].astype(np.uint32), W, H) == np.arange(W * H)).all()
    with pytest.raises(ValueError):
        RI.to_list(frame, H, W)


def test_the_oracle_through_a_degenerate_camera(orc):
    """What tests/test_gpu_ray_image.py holds the kernel to.  Cornell from its own camera: the ray towards the back wall gives pixels that
    differ with the pixel's stream (same ray, another pixel id) and the ray past the box gives the same sky colour under every stream."""
    sc = AC.scene("cornell")
    S = orc.Scene(sc["flat"])
    env = orc.make_env(**sc["env"])
    W, H = 6, 4
    cam = AC.camera(sc, W, H, orc.to_camera_data).as_array()
    o = cam[0:3]
    wall = (cam[3:6] + cam[6:9] * F32(0.5) + cam[9:12] * F32(0.5)).astype(F32)  # through the middle of the image: into the box
    sky = (o + (o - wall)).astype(F32)  # the opposite way: nothing there
    c12, d = RR.degenerate_camera(o, wall)
    assert c12.dtype == F32 and d.dtype == F32 and (d == wall - o).all() and (c12[6:] == 0).all() and (c12[:3] == o).all() and (c12[3:6] == wall).all()
    n = W * H
    for target, varies in ((wall, True), (sky, False)):
        orgs, targets = np.tile(o, (n, 1)), np.tile(target, (n, 1))
        assert (RR.rays_through(orgs, targets)[1] == (target - o).astype(F32)).all()
        rgb, rgba = RR.oracle_pixels(orc, S, env, orgs, targets, W, H, 4, 8)
        assert np.isfinite(rgb).all() and (rgb.reshape(n, 3).max(1) > 0).all()
        distinct = len({p.tobytes() for p in rgb.reshape(n, 3)})
        print("%s: %d distinct pixels of %d" % ("wall" if varies else "sky", distinct, n))
        assert distinct > n // 2 if varies else distinct == 1
        if not varies:
            assert (rgb.reshape(n, 3)[0] == F32(sc["env"]["color"]) * F32(sc["env"]["intensity"])).all()
        # a subset leaves the rest +0, and a pixel does not depend on which others are asked for
        ids = [1, W + 2, n - 1]
        part, part8 = RR.oracle_pixels(orc, S, env, orgs, targets, W, H, 4, 8, ids=ids)
        own = np.zeros(n, bool)
        own[ids] = True
        own = own.reshape(H, W)[::-1]
        assert (part[own].view(np.uint32) == rgb[own].view(np.uint32)).all() and (part8[own] == rgba[own]).all()
        assert (part[~own].view(np.uint32) == 0).all() and (part8[~own] == 0).all()
    # the 1 x 1 form is the camera it names: origin 0, llc = dir, horizontal = du, vertical = dv
    d, du, dv = F32([0.1, -0.2, -1.0]), F32([0.15, 0.0, 0.02]), F32([0.0, 0.12, -0.01])
    got, got8 = RR.oracle_jitter_1x1(orc, S, env, d, du, dv, 16, 8)
    want, want8, _ = S.render(orc.camera_from_array(np.concatenate([np.zeros(3, F32), d, du, dv])), env, 1, 1, 16, 8, want_rgba8=True)
    assert got.shape == (3,) and np.isfinite(got).all() and (got.view(np.uint32) == want[0, 0].view(np.uint32)).all() and got8 == want8[0, 0]


def test_ray_image_kernel_resources():
    """From the Makefile's own target (the flags that ship): the five instances of the translation unit and nothing else - the instrumented
    one, both slab forms of the 4-wave product instance and of its 3-wave fallback - no scratch anywhere, the 4-wave instances within 128
    VGPRs."""
    blocks = resource_report.report("asm-rayimage")[1]
    names = [b[0] for b in blocks]
    assert len(blocks) == 5 and len(set(names)) == 5, names
    assert all("pt_render_rayimage_kernel" in nm for nm in names), "the ray-image translation unit holds the ray-image kernels and no other: %r" % (names,)
    # template arguments <COUNT, WAVES, EXACT> as the Itanium mangling spells them
    want = {"ILb1ELi2ELb0EE", "ILb0ELi4ELb0EE", "ILb0ELi4ELb1EE", "ILb0ELi3ELb0EE", "ILb0ELi3ELb1EE"}
    assert {re.search(r"kernel(I\w+?EE)v", nm).group(1) for nm in names} == want, names
    for nm, vgprs, scratch in blocks:
        assert int(scratch) == 0 and int(vgprs) > 0, (nm, vgprs, scratch)
        if "Li4E" in nm:
            assert int(vgprs) <= 128, (nm, vgprs)


# ---- the oracle's ray-image generator -----------------------------------------------------------------------------------------
ANCHOR_SCENES = ("cornell", "cube", "ico_map")
AW, AH, ASPP, ADEPTH = 20, 13, 4, 8
_oracle = {}


def _oracle_scene(orc, name):
    if name not in _oracle:
        sc = AC.scene(name)
        _oracle[name] = (orc.Scene(sc["flat"]), orc.make_env(**sc["env"]))
    return _oracle[name]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("name", ANCHOR_SCENES)
def test_zero_jitter_is_the_degenerate_camera(orc, name):
    """Origins and directions of the scrambled table (every pixel its own), the jitter zero: dir = fl(L - org) with L = fl(org + dir)."""
    S, env = _oracle_scene(orc, name)
    t = RT.scrambled(name, AW, AH)
    orgs = t["org"].copy()
    targets = (orgs.astype(np.float64) + t["dir"].astype(np.float64)).astype(F32)
    _, dirs = RR.rays_through(orgs, targets)
    table = RI.fixed(orgs, dirs, AW, AH)
    assert (table["dir"] == dirs).all() and (table["org"] == orgs).all()
    cnt = {}
    want, want8 = RR.oracle_pixels(orc, S, env, orgs, targets, AW, AH, ASPP, ADEPTH, counters=cnt)
    assert len({p.tobytes() for p in want.reshape(-1, 3)}) > AW * AH // 3 and cnt["samples"] == AW * AH * ASPP
    for threads in (1, 7):
        rgb, rgba, c = S.render_rays(table, env, AW, AH, ASPP, ADEPTH, threads=threads, want_rgba8=True, want_counters=True)
        assert (_bits(rgb) == _bits(want)).all() and (rgba == want8).all(), threads
        assert c == cnt, (threads, c, cnt)
    # the same records as W * H * 16 plain floats
    flat = np.ascontiguousarray(table).view(F32).copy()
    assert (_bits(S.render_rays(flat, env, AW, AH, ASPP, ADEPTH)[0]) == _bits(want)).all()
    ids = [0, 3, AW + 2, AW * AH - 1, 7 * AW + 19]
    part, part8, c = S.render_rays(table, env, AW, AH, ASPP, ADEPTH, pixel_list=ids, want_rgba8=True, want_counters=True)
    wp, wp8 = RR.oracle_pixels(orc, S, env, orgs, targets, AW, AH, ASPP, ADEPTH, ids=ids)
    assert (_bits(part) == _bits(wp)).all() and (part8 == wp8).all() and c["samples"] == len(ids) * ASPP
    assert (part.reshape(-1, 3).max(1) != 0).sum() <= len(ids)
    with pytest.raises(ValueError):
        S.render_rays(table, env, AW, AH, ASPP, ADEPTH, pixel_list=[AW * AH])
    with pytest.raises(ValueError):
        S.render_rays(table[:-1], env, AW, AH, ASPP, ADEPTH)


@pytest.mark.parametrize("name", ("cornell", "cube"))
def test_jittered_one_pixel_records_are_the_camera_they_name(orc, name):
    import aov_rays_common as ARC

    S, env = _oracle_scene(orc, name)
    seen = set()
    for t in ARC.jitter_records(RT.DTYPE):
        rgb, rgba, c = S.render_rays(t, env, 1, 1, 64, ADEPTH, want_rgba8=True, want_counters=True)
        want, want8 = RR.oracle_jitter_1x1(orc, S, env, t["dir"][0], t["du"][0], t["dv"][0], 64, ADEPTH)
        assert (_bits(rgb[0, 0]) == _bits(want)).all() and rgba[0, 0] == want8 and c["samples"] == 64
        seen.add(want.tobytes())
    assert len(seen) >= 2  # (from the origin some of the eight see the environment alone)


FIRST_RAY_SAMPLES = 8


def _far_scene(orc):
    """One triangle far outside every table: every sample of every pixel misses, so no path draws from the stream."""
    far = dict(positions=F32([[[1e6, 1e6, 1e6], [1e6 + 1, 1e6, 1e6], [1e6, 1e6 + 1, 1e6]]]), normals=F32([[[0, 0, 1]] * 3]), texcoords=None,
               material_index=np.zeros(1, np.int32), texture_index=np.full(1, -1, np.int32), materials=orc.MAT_DEFAULT[None, :], textures=[])
    return orc.Scene(far), orc.make_env(color=(1, 1, 1), intensity=1.0), RT.scrambled_in_box((-1, -2, -3), (3, 2, 1), AW, AH, 77)


def _first_rays(orc, S, env, t, W, H, ns, depth):
    """What the oracle says of the first ns samples of every pixel at `depth`: rays (W * H, ns, 6) = row 0 of each sample's per-bounce log,
    hit (W * H, ns) = its hit flag, rx, ry (W * H, ns) = the two draws from the state the stream was in when the sample began -
    rng_init(x, y) for sample 0, the state trace_pixel_rays reports after sample k - 1 for sample k."""
    n = W * H
    rays, hit = np.zeros((n, ns, 6), F32), np.zeros((n, ns), bool)
    rx, ry = np.zeros((n, ns), F32), np.zeros((n, ns), F32)
    for i in range(n):
        x, y = i % W, i // W
        rgb, after = S.trace_pixel_rays(t, env, W, H, x, y, ns, depth)
        begin = [orc.rng_init(x, y)] + [int(v) for v in after[:-1]]
        for k in range(ns):
            log = S.trace_sample_rays(t, env, W, H, x, y, k, depth)
            assert 1 <= log.shape[0] and log[0, 31] == 0
            rays[i, k], hit[i, k] = log[0, :6], log[0, 6] != 0
            rx[i, k], st = orc.rng_next(begin[k])
            ry[i, k], st = orc.rng_next(st)
    return rays, hit, rx, ry


@pytest.mark.parametrize("what", ("far", "ico_map", "cornell"))
def test_first_ray_is_the_numpy_restatement_and_no_wrong_form_is(orc, what):
    """Row 0 of the per-bounce log (the ray a sample starts on) of EVERY pixel of a scrambled 20 x 13 table, samples 0 to 7 (the issue's
    0, 1 and 7 among them), depth 8, against the numpy restatement: the two draws from the state the stream is in when the sample
    begins, RR.first_sums in float32 and aov_rays_ref.normalize3 - bit for bit.  A path draws from the pixel's stream at every hit, so
    sample k > 0 begins where sample k - 1 ended (Scene.trace_pixel_rays, behind the one trace_path that tests/test_oracle_vs_reference.py
    holds to the reference), not at draw 2k.  aov_rays_ref.table_rays, the restatement the guide pass is held to, does put sample k at
    draws 2k and 2k + 1: it is compared on sample 0 of every pixel, on the later samples of the pixels whose earlier samples all missed,
    and on everything in the scene where every sample misses ("far").  Then the mistakes a generator could make (RR.FORMS): each differs
    from the oracle."""
    n, ns = AW * AH, FIRST_RAY_SAMPLES
    S, env, t = _far_scene(orc) if what == "far" else _oracle_scene(orc, what) + (RT.scrambled(what, AW, AH),)
    rays, hit, rx, ry = _first_rays(orc, S, env, t, AW, AH, ns, ADEPTH)
    assert (_bits(rays[..., :3]) == _bits(t["org"])[:, None, :]).all()
    jittered = t["du"].any(1) | t["dv"].any(1)
    both = t["du"].any(1) & t["dv"].any(1)
    assert len({r.tobytes() for r in t["du"][both]}) == both.sum() > n // 2 and (rx != ry).all()
    for form in RR.FORMS:
        differ = np.zeros((n, ns), bool)
        for k in range(ns):
            with np.errstate(invalid="ignore", divide="ignore"):
                d = aov_rays_ref.normalize3(RR.first_sums(t, rx[:, k], ry[:, k], form))
            differ[:, k] = (_bits(d) != _bits(rays[:, k, 3:])).any(1)
        print("%s, form %-9s: %4d of %d directions differ from the oracle's" % (what, form, differ.sum(), differ.size))
        if form == "right":
            assert not differ.any()
        elif form == "dv_first":  # the same terms in another order: a rounding apart where both are there, and nothing otherwise
            assert not differ[~both].any() and differ[both].any()
        else:  # another record's jitter, or the other draw: every jittered record shows it
            assert differ[jittered].all()
    # table_rays: where the stream is at draw 2k
    want = aov_rays_ref.table_rays(t, AW, AH, ns, np.arange(n))
    clean = np.concatenate([np.ones((n, 1), bool), np.cumsum(hit, 1)[:, :-1] == 0], 1)  # no sample in front drew from the stream
    print("%s: samples at draw 2k per position 0..7: %s" % (what, clean.sum(0).tolist()))
    if what == "far":
        assert not hit.any() and clean.all()
        d_rx, d_ry = RR.draws(orc, AW, AH, ns)
        assert (d_rx == rx).all() and (d_ry == ry).all()
    else:
        assert clean[:, 0].all() and not clean[:, 1].all()
    same = (_bits(rays) == _bits(want)).all(-1)
    assert same[clean].all(), "%s: %d first rays differ from table_rays" % (what, int((~same[clean]).sum()))
    with pytest.raises(RuntimeError):
        S.trace_sample_rays(t, env, AW, AH, AW, 0, 0, 1)
    with pytest.raises(RuntimeError):
        S.trace_pixel_rays(t, env, AW, AH, 0, AH, 1, 1)


@pytest.mark.parametrize("name", ANCHOR_SCENES)
def test_a_wrong_generator_differs_from_the_oracle_as_a_frame(orc, name):
    """At 1 spp the frame of a table under a generator of some form is the frame of the zero-jitter table that holds that form's sum of
    sample 0 (RR.one_sample_table).  The right form gives Scene.render_rays of the jittered table bit for bit - the generator anchored
    once more, at W, H > 1 with jitter, through the zero-jitter identity above - and every wrong form gives another frame: a kernel
    with that mistake would fail the GPU legs, which compare every pixel."""
    S, env = _oracle_scene(orc, name)
    t = RT.scrambled(name, AW, AH)
    rx, ry = RR.draws(orc, AW, AH, 1)
    want = S.render_rays(t, env, AW, AH, 1, ADEPTH)[0]
    shares = {}
    for form in RR.FORMS:
        got = S.render_rays(RR.one_sample_table(t, rx[:, 0], ry[:, 0], form), env, AW, AH, 1, ADEPTH)[0]
        shares[form] = RT.differing_share(got, want)
    print(name, shares)
    assert shares["right"] == 0.0
    for form in RR.FORMS:
        if form != "right":
            assert shares[form] > 0.0, "the form '%s' (%s) gives the oracle's frame" % (form, RR.FORMS[form])


def test_reserved_floats_are_not_read(orc):
    S, env = _oracle_scene(orc, "cornell")
    t = RT.scrambled("cornell", AW, AH)
    assert all(np.isnan(t["reserved%d" % k]).all() for k in range(4))
    z = t.copy()
    other = t.copy()
    for k in range(4):
        z["reserved%d" % k] = 0.0
        other["reserved%d" % k] = F32(k + 1) * F32(1e30)
    a = S.render_rays(t, env, AW, AH, ASPP, ADEPTH, want_rgba8=True, want_counters=True)
    for b in (S.render_rays(z, env, AW, AH, ASPP, ADEPTH, want_rgba8=True, want_counters=True), S.render_rays(other, env, AW, AH, ASPP, ADEPTH, want_rgba8=True, want_counters=True)):
        assert (_bits(a[0]) == _bits(b[0])).all() and (a[1] == b[1]).all() and a[2] == b[2]
    assert np.isfinite(a[0]).all()
    la, lz = S.trace_sample_rays(t, env, AW, AH, 5, 4, 2, ADEPTH), S.trace_sample_rays(z, env, AW, AH, 5, 4, 2, ADEPTH)
    assert la.shape == lz.shape and (_bits(la) == _bits(lz)).all()


def test_scrambled_table_is_what_it_says():
    for name, W, H in (("cornell", 64, 48), ("ico_map", 64, 48), ("cube", 20, 13)):
        t = RT.scrambled(name, W, H)
        assert t.dtype == RT.DTYPE == B.RAY_GEN_DTYPE and t.shape == (W * H,) and not t.flags.writeable
        assert RT.scrambled(name, W, H) is t and RT.scrambled_in_box((0, 0, 0), (1, 1, 1), 3, 2, 5).tobytes() == RT.scrambled_in_box((0, 0, 0), (1, 1, 1), 3, 2, 5).tobytes()
        lo, hi = RT.box_of(AC.scene(name)["flat"])
        u = (t["org"].astype(np.float64) - lo) / (hi - lo)
        assert u.min() >= 0.1 - 1e-6 and u.max() <= 0.9 + 1e-6 and u.std(0).min() > 0.15
        for c, r in RT.DARK.get(name, ()):
            assert (np.linalg.norm(t["org"] - F32(c), axis=1) >= r - 1e-5).all()
        ln = np.linalg.norm(t["dir"].astype(np.float64), axis=1)
        assert ln.min() >= 0.5 - 1e-6 and ln.max() <= 2.0 + 1e-6
        for f in ("du", "dv"):
            r = np.linalg.norm(t[f].astype(np.float64), axis=1) / ln
            zero = r == 0
            assert 0.15 < zero.mean() < 0.35  # an eighth alone and an eighth with the other
            assert r[~zero].min() >= 0.05 - 1e-6 and r[~zero].max() <= 0.5 + 1e-6
        both = ~t["du"].any(1) & ~t["dv"].any(1)
        assert 0.06 < both.mean() < 0.2
        assert all(np.isnan(t["reserved%d" % k]).all() for k in range(4))
        for f in ("org", "dir", "du", "dv"):
            assert np.isfinite(t[f]).all()
    for name, (c, r) in RT.ONLY.items():
        t = RT.scrambled(name, 20, 13)
        assert (np.linalg.norm(t["org"].astype(np.float64) - c, axis=1) < r).all() and t["org"].std(0).min() > 0.2 * r
    one = RT.scrambled("cornell", 1, 1)
    assert one["du"].any() and one["dv"].any()
    # the three wrong tables
    t = RT.scrambled("cube", 20, 13)
    nb, z, ex = RT.neighbour(t), RT.zeroed(t), RT.exchanged(t)
    assert (nb["du"][1:] == t["du"][:-1]).all() and (nb["dv"][0] == t["dv"][-1]).all() and (nb["dir"] == t["dir"]).all() and (nb["org"] == t["org"]).all()
    assert not z["du"].any() and not z["dv"].any() and (z["dir"] == t["dir"]).all()
    assert (ex["du"] == t["dv"]).all() and (ex["dv"] == t["du"]).all()
    p = RI.pinhole(AC.camera(AC.scene("cornell"), 8, 6, B.to_camera_data), 8, 6)
    assert RT.neighbour(p).tobytes() == p.tobytes(), "a pinhole table rolled is the same table: why it cannot tell records apart"
    e = RT.equirect("cornell", 16, 8)
    assert (np.linalg.norm(e["du"][:16], axis=1) < 0.5 * np.linalg.norm(e["du"][4 * 16:5 * 16], axis=1)).all(), "the jitter shrinks towards the poles"


RAY_SIZES = ((1, 1), (7, 9), (20, 13), (64, 48), (130, 3), (3, 130))


@pytest.mark.parametrize("kind", ("scrambled", "equirect"))
@pytest.mark.parametrize("name", ANCHOR_SCENES)
def test_tables_meet_their_precondition(orc, name, kind):
    """With the oracle alone, at every (scene, table, size, spp) the GPU legs of tests/test_gpu_ray_image.py use (they assert it again on
    the frames they compare): the figures in the docstring of tests/ray_tables.py."""
    S, env = _oracle_scene(orc, name)
    for W, H in RAY_SIZES:
        if kind == "equirect" and W * H == 1:
            continue
        for spp in (4, 64):
            out = RT.precondition(S, env, RT.table(kind, name, W, H), W, H, spp, ADEPTH)
            print("%-9s %-7s %3d x %-3d %2d spp: %s" % (kind, name, W, H, spp, "  ".join("%s %.1f %%" % (k, 100 * v) for k, v in out.items())))
