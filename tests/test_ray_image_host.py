"""Ray images (pt_render_rays; include/mi355pt.h "ray images") without a GPU.

* The two exports exist, are in B.EXPORTS and in the header, the record is 64 bytes with the fields where the header puts them, the ABI
  version is still 5 and the _device form is in both lists of the streams contract.
* Every refusal of the header on a host-only context, by code and by message; a refused call writes nothing.  (A communicator needs a
  device: that refusal is tests/test_gpu_ray_image.py's.)
* pyhost/ray_image.py: pinhole against gen_camera_ray's formula in float64, equirect against its formula, fixed and to_list.
* tests/ray_image_ref.py itself: through a degenerate camera the oracle's pixel depends on the pixel's stream on a diffuse wall and not on
  sky, and the 1 x 1 form is the camera it names.
* `make asm-rayimage`: exactly the five instances, no scratch, the 4-wave instances within 128 VGPRs."""
import ctypes as C
import re

import numpy as np
import pytest

import aov_common as AC
import ray_image_ref as RR
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
