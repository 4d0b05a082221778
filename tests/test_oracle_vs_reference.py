"""The oracle against the reference's own device code.

oracle/_ref/libref_device.so is the reference's random.hpp, math.hpp, sample_methods.hpp, disney/ headers and device.cu
compiled for the CPU against stand-in headers for OWL / OptiX / CUDA (oracle/ref_shim/ref_shim.h says what those define:
traversal, texture filtering, make_rgba, the vector library, and the transcendentals, which both twins share).  Every
formula, constant, branch, RNG draw and the path loop run as the reference wrote them, so these tests pin what no
reference output pins: clearcoat, rough glass, sheen, the oblique and anisotropic rough specular lobe,
Russian roulette and the bookkeeping of trace_path / ray_gen.  The HIP path equals the oracle bit for bit
(tests/test_gpu_*.py), so it is pinned through the oracle.

Where the twins do the same arithmetic they agree bit for bit, and the tests say so.  They differ only where the oracle
fuses a multiply-add that the reference writes as two operations (the oracle's model of nvcc's contraction): lerp
(math.hpp:6-10), the barycentric sums (device.cu:59,72,86) and to_world (math.hpp:104-107).  Quantities downstream of
those are compared to a few ulp; the clearcoat sample, whose GTR1 inversion amplifies a one-ulp change of its alpha,
to a few hundred; path radiance, which compounds them over the bounces, to 1e-4 relative.  A transcription error moves
values by far more than that, or changes the RNG stream.
"""
import numpy as np
import pytest

from conftest import ASSETS

LOBE_NONE, LOBE_DIFFUSE, LOBE_CLEARCOAT, LOBE_METALLIC, LOBE_GLASS = -1, 0, 1, 2, 3


@pytest.fixture(scope="module")
def ref():
    import reference

    if not reference.available():
        pytest.skip("oracle/_ref/libref_device.so is not built: build() makes it where a reference checkout is readable "
                    "(PT_REFERENCE_DIR)")
    reference.lib()
    return reference


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


def _same(a, b):
    return np.array_equal(np.atleast_1d(np.float32(a)), np.atleast_1d(np.float32(b)), equal_nan=True)


def _assert_close(got, want, ulps=0, atol=0.0, rtol=0.0, what=""):
    """Equal, or within `ulps` units in the last place of `want`, rtol of it, or atol (for components near 0)."""
    g = np.atleast_1d(np.asarray(got, np.float32)).astype(np.float64)
    w = np.atleast_1d(np.asarray(want, np.float32))
    with np.errstate(invalid="ignore"):  # inf - inf
        err = np.abs(g - w.astype(np.float64))
        tol = np.maximum(np.maximum(ulps * np.spacing(np.abs(w)).astype(np.float64), rtol * np.abs(w)), atol)
        ok = (g == w) | (np.isnan(g) & np.isnan(w)) | (err <= tol)
    assert ok.all(), "%s: oracle %r vs reference %r (ulp %s, rtol %s, atol %s allowed)" % (what, got, want, ulps, rtol, atol)


def _directions(rng, n):
    """Random unit vectors in both hemispheres, with poles, the horizon and near-grazing ones mixed in."""
    out = [_unit([0, 0, 1]), _unit([0, 0, -1]), _unit([1, 0, 0]), _unit([0.3, -0.4, 1e-3]), _unit([-0.2, 0.1, -2e-3])]
    while len(out) < n:
        v = rng.normal(size=3)
        if rng.uniform() < 0.15:
            v[2] *= 1e-2
        out.append(_unit(v))
    return out


def _materials(rng, n, scene_io):
    """Random material_data covering every lobe and weight, each feature switched off in part of the draws."""
    out = []
    for _ in range(n):
        pick = lambda p=0.5: float(rng.uniform()) if rng.uniform() < p else 0.0  # noqa: E731
        out.append(scene_io.material(
            base_color=rng.uniform(0, 1, 3), metallic=pick(), specular=float(rng.uniform()), specular_tint=float(rng.uniform()),
            roughness=float(rng.choice([0.0, 1.0, rng.uniform()])), anisotropic=pick(), sheen=pick(), sheen_tint=float(rng.uniform()),
            clearcoat=pick(), clearcoat_gloss=float(rng.uniform()), ior=float(rng.uniform(1.0, 2.4)),
            specular_transmission=float(rng.choice([0.0, 1.0, rng.uniform()])),
            specular_transmission_roughness=float(rng.choice([0.0, rng.uniform()]))))
    return out


def test_rng_streams_identical(orc, ref):
    # random.hpp:46-69: TEA seeding and the LCG, the integer state and the float draw
    for u in (0, 1, 7, 1919, 1079, 0x7FFFFFFF, 0xFFFFFFFF):
        for v in (0, 3, 1080, 0xFFFFFFFF):
            s_o, s_r = orc.rng_init(u, v), ref.rng_init(u, v)
            assert s_o == s_r
            for _ in range(8):
                f_o, s_o = orc.rng_next(s_o)
                f_r, s_r = ref.rng_next(s_r)
                assert s_o == s_r and f_o == f_r


def test_frame_and_sampling_helpers(orc, ref):
    # math.hpp:58-107, sample_methods.hpp:19-65, device.cu:23-28
    rng = np.random.default_rng(11)
    normals = _directions(rng, 300) + [_unit([1, 1, 1]), _unit([-1, -1, -1])]  # the (-1,1,1) x N branch of onb
    for n in normals:
        t_o, b_o = orc.onb(n)
        t_r, b_r = ref.onb(n)
        assert _same(t_o, t_r) and _same(b_o, b_r), n
        w = _unit(rng.normal(size=3))
        assert _same(orc.to_local(t_o, b_o, n, w), ref.to_local(t_r, b_r, n, w))
        # the oracle fuses w.x t + w.y b + w.z n
        _assert_close(orc.to_world(t_o, b_o, n, w), ref.to_world(t_r, b_r, n, w), 4, atol=3e-7, what="to_world")
        assert _same(orc.uv_on_sphere(n), ref.uv_on_sphere(n)), n
    for u0, u1 in [(0.5, 0.5), (0.0, 0.0), (1.0, 1.0), (0.5, 0.9), (0.1, 0.5)] + [tuple(x) for x in rng.uniform(0, 1, (300, 2))]:
        assert _same(orc.sample_cosine_hemisphere(u0, u1), ref.sample_cosine_hemisphere(u0, u1)), (u0, u1)
    for w in _directions(rng, 200):
        m = _unit(rng.normal(size=3))
        for eta in (1.0, 1 / 1.5, 1.5, 2.4, float(rng.uniform(0.4, 2.5))):
            ok_o, wi_o = orc.refract(w, m, eta)
            ok_r, wi_r = ref.refract(w, m, eta)
            assert ok_o == ok_r and (not ok_o or _same(wi_o, wi_r)), (w, m, eta)
            assert _same(orc.fresnel_equation(w, m, 1.0, eta), ref.fresnel_equation(w, m, 1.0, eta))
            assert _same(orc.fresnel_equation(w, m, eta, 1.0), ref.fresnel_equation(w, m, eta, 1.0))  # with total internal reflection


def test_microfacet_terms_identical(orc, ref):
    # disney_specular.cuh:17-60 (anisotropic GGX and its Smith lambda), disney_clearcoat.cuh:13-20 (GTR1)
    rng = np.random.default_rng(12)
    for w in _directions(rng, 400):
        ax, ay = (float(a) for a in rng.choice([0.001, 1.0, rng.uniform(0.001, 1.0)], 2))
        assert _same(orc.lambda_(w, ax, ay), ref.lambda_(w, ax, ay)), (w, ax, ay)
        assert _same(orc.d_gtr2(w, ax, ay), ref.d_gtr2(w, ax, ay)), (w, ax, ay)
        for alpha in (0.001, 0.0505, 0.1, float(rng.uniform(0.001, 1.0)), 1.0, 1.3):
            assert _same(orc.d_gtr1(w, alpha), ref.d_gtr1(w, alpha)), (w, alpha)


# ulp allowed per lobe for eval: 0 where no lerp is involved
EVAL_ULPS = {LOBE_DIFFUSE: 0, LOBE_CLEARCOAT: 8, LOBE_METALLIC: 8, LOBE_GLASS: 0}


@pytest.mark.parametrize("lobe", [LOBE_DIFFUSE, LOBE_CLEARCOAT, LOBE_METALLIC, LOBE_GLASS], ids=["diffuse", "clearcoat", "metallic", "glass"])
def test_lobe_eval_matches_reference(orc, ref, scene_io, lobe):
    # disney_diffuse.cuh:26-55, disney_clearcoat.cuh:45-59, disney_specular.cuh:125-149 and :193-214, at arbitrary
    # (wo, wh, wi) in both hemispheres: oblique and anisotropic specular, rough glass reflection and transmission
    rng = np.random.default_rng(20 + lobe)
    mats = _materials(rng, 64, scene_io)
    dirs = _directions(rng, 64)
    n = 0
    for i in range(1500):
        m = mats[i % len(mats)]
        wo = dirs[i % len(dirs)]
        wi = dirs[(7 * i + 3) % len(dirs)]
        wh = _unit(wo.astype(np.float64) + wi) if rng.uniform() < 0.7 else _unit(rng.normal(size=3))
        f_o, pdf_o = orc.eval_lobe(lobe, m, wo, wh, wi)
        f_r, pdf_r = ref.eval_lobe(lobe, m, wo, wh, wi)
        _assert_close(f_o, f_r, EVAL_ULPS[lobe], what="f")
        _assert_close(pdf_o, pdf_r, EVAL_ULPS[lobe], what="pdf")
        n += int(np.isfinite(f_r).all() and (f_r != 0).any())
    assert n > 300  # mostly non-trivial values


def test_sheen_matches_reference(orc, ref, scene_io):
    # disney_sheen.cuh:15-37 (the tint lerp is the only fused step)
    rng = np.random.default_rng(30)
    mats = _materials(rng, 64, scene_io)
    dirs = _directions(rng, 64)
    nonzero = 0
    for i in range(1500):
        m = mats[i % len(mats)]
        wo, wi = dirs[i % len(dirs)], dirs[(5 * i + 1) % len(dirs)]
        f_r = ref.eval_sheen(m, wo, wi)
        _assert_close(orc.eval_sheen(m, wo, wi), f_r, 8, what="sheen")
        nonzero += int(f_r.any())
    assert nonzero > 300
    m = mats[0].copy()
    m[9] = 0.6
    assert not ref.eval_sheen(m, dirs[5], -dirs[5]).any() and not orc.eval_sheen(m, dirs[5], -dirs[5]).any()  # degenerate wh


def test_sample_disney_matches_reference(orc, ref, scene_io):
    # disney.cuh:15-66 with every lobe's sampler: the chosen lobe and the RNG state after the call are exact, as are wi and
    # pdf outside the clearcoat lobe; f carries the lerp of the specular tint / sheen
    rng = np.random.default_rng(40)
    mats = _materials(rng, 256, scene_io)
    dirs = _directions(rng, 128)
    seen = set()
    for i in range(12000):
        m = mats[i % len(mats)]
        wo = dirs[(3 * i) % len(dirs)]
        state = int(rng.integers(0, 2 ** 32))
        lobe_in = int(rng.choice([LOBE_NONE, LOBE_DIFFUSE, LOBE_CLEARCOAT, LOBE_METALLIC, LOBE_GLASS]))  # GLASS + wo.z < 0: force_btdf
        a = orc.sample_disney(m, wo, state, lobe_in)
        b = ref.sample_disney(m, wo, state, lobe_in)
        ctx = "material %s wo %s state %d lobe %d" % (m.tolist(), wo.tolist(), state, lobe_in)
        assert a["lobe"] == b["lobe"], ctx
        assert a["state"] == b["state"], ctx  # same number and order of draws
        if b["lobe"] == LOBE_CLEARCOAT:
            _assert_close(a["wi"], b["wi"], 256, atol=2e-6, what="clearcoat wi " + ctx)
            _assert_close(a["pdf"], b["pdf"], 512, what="clearcoat pdf " + ctx)
            _assert_close(a["f"], b["f"], 512, what="clearcoat f " + ctx)
        else:
            assert _same(a["wi"], b["wi"]), ctx
            assert _same(a["pdf"], b["pdf"]), ctx
            _assert_close(a["f"], b["f"], 8, what="f " + ctx)
        seen.add((b["lobe"], wo[2] < 0))
    assert {(lb, False) for lb in (LOBE_DIFFUSE, LOBE_CLEARCOAT, LOBE_METALLIC, LOBE_GLASS)} <= seen
    assert (LOBE_GLASS, True) in seen


def _all_lobes_scene(scene_io):
    """The cornell box with a material per lobe mix: sheen + clearcoat over diffuse, rough glass, anisotropic rough metal,
    clearcoated metal, and a half-transmissive rough mix; the light keeps its emission."""
    sc = scene_io.load_scene_dir(ASSETS, "cornell-box")
    flat = scene_io.flatten_scene(sc["entities"], sc["materials"])
    by_name = {
        "box": scene_io.material(base_color=[0.7, 0.6, 0.5], roughness=0.6, sheen=0.8, sheen_tint=0.5, clearcoat=0.7, clearcoat_gloss=0.4),
        "sphere": scene_io.material(base_color=[0.9, 0.95, 1.0], specular_transmission=1.0, specular_transmission_roughness=0.35,
                                    roughness=0.3, ior=1.5),
        "wall_left": scene_io.material(base_color=[0.9, 0.6, 0.3], metallic=1.0, roughness=0.45, anisotropic=0.7),
        "wall_right": scene_io.material(base_color=[0.2, 0.7, 0.3], metallic=0.4, roughness=0.3, clearcoat=1.0, clearcoat_gloss=0.9,
                                        sheen=0.3),
        "wall_tbb": scene_io.material(base_color=[0.8, 0.2, 0.2], specular_transmission=0.5, roughness=0.7,
                                      specular_transmission_roughness=0.8, sheen=0.5),
    }
    mats = np.asarray(flat["materials"], np.float32).copy()
    for i, (name, _, _) in enumerate(sc["materials"]):
        if name in by_name:
            mats[i] = by_name[name]
    assert mats[:, 16].any()  # the light
    flat["materials"] = mats
    return sc, flat


def _envs(orc, scene_io):
    return {
        "color": orc.make_env(color=(0.3, 0.35, 0.4), intensity=1.0),
        "auto": orc.make_env(use_auto=True, intensity=0.7),
        "map": orc.make_env(use_map=True, env_map=scene_io.checker_texture(16, 8, 2), intensity=2.0),
    }


@pytest.mark.parametrize("env_kind", ["color", "auto", "map"])
def test_trace_path_matches_reference(orc, ref, scene_io, env_kind):
    # device.cu:113-218 per sample: hit / miss / emission, the pdf cut-off, throughput, Russian roulette (depth > 3, not after
    # glass, q = max(.05, 1 - max throughput)); the RNG state after every sample is exact, the radiance within 1e-4
    sc, flat = _all_lobes_scene(scene_io)
    S, R = orc.Scene(flat), ref.Scene(flat)
    assert R.meshes == len(sc["materials"])
    env = _envs(orc, scene_io)[env_kind]
    c = sc["camera"]
    W = H = 32
    spp, depth = 8, 16
    cam = orc.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H)
    lobes, long_paths = set(), 0
    for py in range(1, H, 3):
        for px in range(2, W, 3):
            rgb_o, st_o = S.trace_pixel(cam, env, W, H, px, py, spp, depth)
            rgb_r, st_r = R.trace_pixel(cam, env, W, H, px, py, spp, depth)
            np.testing.assert_array_equal(st_o, st_r, err_msg="pixel (%d, %d)" % (px, py))
            _assert_close(rgb_o, rgb_r, rtol=1e-4, atol=1e-7, what="pixel (%d, %d)" % (px, py))
            if px % 9 == 2 and py % 9 == 1:
                log = S.trace_sample(cam, env, W, H, px, py, spp - 1, depth)
                lobes |= {int(x) for x in log[:, 23].view(np.int32) if log.size}
                long_paths += int(len(log) > 4)
    # the scene reaches every lobe and paths long enough for the roulette
    assert {LOBE_DIFFUSE, LOBE_CLEARCOAT, LOBE_METALLIC, LOBE_GLASS} <= lobes
    assert long_paths > 0


def _white_box(scene_io):
    """The cornell box with every surface but the light a white, fully rough diffuser: the throughput stays near or above
    0.95, so nearly every path reaches the roulette with q at its floor of 0.05 (device.cu:212)."""
    sc = scene_io.load_scene_dir(ASSETS, "cornell-box")
    flat = scene_io.flatten_scene(sc["entities"], sc["materials"])
    mats = np.asarray(flat["materials"], np.float32).copy()
    white = scene_io.material(base_color=[1.0, 1.0, 1.0], roughness=1.0)
    for i in range(len(mats)):
        if mats[i, 16] <= 0:
            mats[i] = white
    flat["materials"] = mats
    return sc, flat


@pytest.mark.parametrize("scene,env_kind", [("all_lobes", "color"), ("all_lobes", "auto"), ("all_lobes", "map"), ("white_box", "color")])
def test_ray_gen_matches_reference(orc, ref, scene_io, scene, env_kind):
    # device.cu:220-254 whole frames: per-pixel stream, jitter, average, the row flip of the framebuffer and the RGBA8 write
    sc, flat = (_all_lobes_scene if scene == "all_lobes" else _white_box)(scene_io)
    S, R = orc.Scene(flat), ref.Scene(flat)
    env = _envs(orc, scene_io)[env_kind]
    c = sc["camera"]
    W, H = 40, 24
    cam = orc.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H)
    want, want8, _ = S.render(cam, env, W, H, 6, 16, want_rgba8=True)
    got, got8 = R.render(cam, env, W, H, 6, 16)
    _assert_close(want, got, rtol=1e-4, atol=1e-7, what="frame")
    np.testing.assert_array_equal(want8, got8)
    assert want.any()


def test_textured_scene_matches_reference(orc, ref, cube):
    # device.cu:75-94 and :170-173: texture coordinates interpolated per hit, tex2D's colour replaces base_color
    flat = cube["flat"]
    assert (np.asarray(flat["texture_index"]) >= 0).any()
    S, R = orc.Scene(flat), ref.Scene(flat)
    c = cube["camera"]
    W = H = 32
    cam = orc.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H)
    env = orc.make_env(use_auto=True, intensity=1.0)
    want, want8, _ = S.render(cam, env, W, H, 8, 8, want_rgba8=True)
    got, got8 = R.render(cam, env, W, H, 8, 8)
    _assert_close(want, got, rtol=1e-4, atol=1e-7, what="frame")
    np.testing.assert_array_equal(want8, got8)
    for py in range(0, H, 5):
        for px in range(0, W, 5):
            np.testing.assert_array_equal(S.trace_pixel(cam, env, W, H, px, py, 8, 8)[1], R.trace_pixel(cam, env, W, H, px, py, 8, 8)[1])
