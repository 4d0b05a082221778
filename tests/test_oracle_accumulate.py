"""The oracle continues a pixel: Scene.accumulate (orc_accumulate) against Scene.render and Scene.trace_pixel, which start at sample 0.
Cornell at 24 x 16, depth 4 (no Russian roulette below depth 4, so a change of base colour leaves every RNG stream alone), environment
use_auto = 1.  Every comparison is bit for bit.

1. For three splits of N = 12 (1 + 11, 5 + 7, 4 + 4 + 4): sum * (1.0f / N) equals render(N), RGBA8 included, and rng equals trace_pixel's
   per_sample_state[N - 1].  The same for a pixel_list; pixels that are not listed keep rng and sum.
2. A split with set_materials between the parts equals, per pixel, the float32 fold of trace_pixel's per-sample radiance: the first k
   samples from the first table, the others from the second - on the pixels whose stream after k samples is the same under both tables
   (all of them here; asserted) - and differs from both unsplit renders.  set_watertight between the parts likewise.
3. What the call refuses."""
import numpy as np
import pytest

F32, U32 = np.float32, np.uint32
W, H, DEPTH, N = 24, 16, 4, 12
ENV = dict(use_auto=True, intensity=1.0)
SPLITS = ((1, 11), (5, 7), (4, 4, 4))


def _cam(orc, cornell):
    """The scene's camera, half way to what it looks at: the box fills most of the frame (a material change shows nowhere in the sky)."""
    c = cornell["camera"]
    frm = 0.5 * (np.asarray(c["look_from"], np.float64) + np.asarray(c["look_at"], np.float64))
    return orc.to_camera_data([float(x) for x in frm], c["look_at"], c["look_up"], c["vertical_fov"], W, H)


def _fresh():
    """State arrays with a pattern no sample writes: `first` must not read them, and an unlisted pixel must keep them."""
    return np.full(W * H, 0xDEADBEEF, U32), np.full(W * H * 3, -7.25, F32)


def _image(sum_, n):
    """launch-order sums -> render's frame: sum * (1.0f / n), rows flipped"""
    return (sum_.reshape(H, W, 3) * (F32(1.0) / F32(n))).astype(F32)[::-1]


def _bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


@pytest.fixture(scope="module")
def S(orc, cornell):
    return orc.Scene(cornell["flat"])


@pytest.fixture(scope="module")
def tables(cornell):
    a = np.stack([m for _, m, _ in cornell["materials"]]).astype(F32)
    b = a.copy()
    b[:, 0:3] = (a[:, [2, 0, 1]] * F32(0.5) + F32(0.2)).astype(F32)  # other base colours in every row, nothing else
    return a, b


@pytest.fixture(scope="module")
def rendered(orc, cornell, S, tables):
    """render(N) under both tables, once"""
    out = []
    for t in tables:
        S.set_materials(t)
        rgb, rgba8, _ = S.render(_cam(orc, cornell), orc.make_env(**ENV), W, H, N, DEPTH, want_rgba8=True)
        rgb.setflags(write=False)
        out.append((rgb, rgba8))
    S.set_materials(tables[0])
    return out


@pytest.mark.parametrize("split", SPLITS)
def test_splits_equal_render(orc, cornell, S, tables, rendered, split):
    cam, env = _cam(orc, cornell), orc.make_env(**ENV)
    S.set_materials(tables[0])
    rng, sum_ = _fresh()
    for k, n in enumerate(split):
        S.accumulate(cam, env, W, H, n, DEPTH, rng, sum_, first=(k == 0), threads=1 + 3 * k)
    want, want8 = rendered[0]
    got = _image(sum_, N)
    assert (_bits(got) == _bits(want)).all(), "%s: %d floats differ" % (split, int((_bits(got) != _bits(want)).sum()))
    assert ([[orc.make_rgba(got[r, x]) for x in range(W)] for r in range(0, H, 5)] == want8[0:H:5].tolist())
    for px, py in ((0, 0), (W - 1, H - 1), (7, 9), (13, 4)):
        _, st = S.trace_pixel(cam, env, W, H, px, py, N, DEPTH)
        assert rng[px + W * py] == st[N - 1], (px, py)
    assert (want > 0).mean() > 0.9


def test_pixel_list_and_untouched_pixels(orc, cornell, S, tables, rendered):
    cam, env = _cam(orc, cornell), orc.make_env(**ENV)
    S.set_materials(tables[0])
    ids = np.random.default_rng(3).permutation(W * H)[: W * H // 3].astype(U32)  # unsorted, as a compacted active set is
    listed = np.zeros(W * H, bool)
    listed[ids] = True
    rng, sum_ = _fresh()
    S.accumulate(cam, env, W, H, 5, DEPTH, rng, sum_, pixel_list=ids, first=True)
    assert (rng[~listed] == 0xDEADBEEF).all() and (sum_.reshape(-1, 3)[~listed] == F32(-7.25)).all()
    mid_rng, mid_sum = rng.copy(), sum_.copy()
    half = ids[: ids.size // 2]
    S.accumulate(cam, env, W, H, 7, DEPTH, rng, sum_, pixel_list=half)  # continue one half of them ...
    second = np.zeros(W * H, bool)
    second[half] = True
    assert (rng[~second] == mid_rng[~second]).all() and (_bits(sum_).reshape(-1, 3)[~second] == _bits(mid_sum).reshape(-1, 3)[~second]).all()
    assert (rng[second] != mid_rng[second]).all()
    S.accumulate(cam, env, W, H, 7, DEPTH, rng, sum_, pixel_list=ids[ids.size // 2:])  # ... then the other
    got, want = _image(sum_, N), rendered[0][0]
    mask = listed.reshape(H, W)[::-1]
    assert (_bits(got)[mask] == _bits(want)[mask]).all()
    assert (rng[~listed] == 0xDEADBEEF).all() and (sum_.reshape(-1, 3)[~listed] == F32(-7.25)).all()
    S.accumulate(cam, env, W, H, 3, DEPTH, rng, sum_, pixel_list=np.zeros(0, U32))  # an empty list: nothing
    assert (_bits(_image(sum_, N))[mask] == _bits(want)[mask]).all()


def _fold(parts):
    """float32 left fold of per-sample radiance rows, as the sample loop adds them"""
    acc = np.zeros(3, F32)
    for r in parts:
        acc = (acc + r).astype(F32)
    return acc


@pytest.mark.parametrize("k", [1, 5])
def test_set_materials_between_the_parts(orc, cornell, S, tables, rendered, k):
    cam, env = _cam(orc, cornell), orc.make_env(**ENV)
    a, b = tables
    S.set_materials(a)
    rng, sum_ = _fresh()
    S.accumulate(cam, env, W, H, k, DEPTH, rng, sum_, first=True)
    S.set_materials(b)
    S.accumulate(cam, env, W, H, N - k, DEPTH, rng, sum_)
    got = _image(sum_, N)
    for t, (want, _) in zip((a, b), rendered):
        # (how many pixels differ has no bound of its own: at depth 4 a sample that has not left the box contributes 0 under any table)
        assert (_bits(got) != _bits(want)).any(), "the split frame must differ from both unsplit ones"
    checked = 0
    for px, py in ((0, 0), (W - 1, H - 1), (7, 9), (13, 4), (3, 12), (20, 2), (11, 7)):
        S.set_materials(a)
        rgb_a, st_a = S.trace_pixel(cam, env, W, H, px, py, N, DEPTH)
        S.set_materials(b)
        rgb_b, st_b = S.trace_pixel(cam, env, W, H, px, py, N, DEPTH)
        if st_a[k - 1] != st_b[k - 1]:
            continue  # the first part moved the stream: the second table's samples from sample 0 are not this pixel's continuation
        checked += 1
        want = _fold(list(rgb_a[:k]) + list(rgb_b[k:]))
        assert (_bits(sum_.reshape(-1, 3)[px + W * py]) == _bits(want)).all(), (px, py)
        assert rng[px + W * py] == st_b[N - 1], (px, py)
    assert checked >= 5, checked
    S.set_materials(a)


def test_set_watertight_between_the_parts(orc, cornell, S, tables):
    """The second part runs the other triangle test: per pixel the fold of the first k samples of the one and the others of the other, where
    the stream after k samples is the same under both (the tests agree on nearly every hit of this scene)."""
    cam, env = _cam(orc, cornell), orc.make_env(**ENV)
    S.set_materials(tables[0])
    k = 5
    try:
        rng, sum_ = _fresh()
        S.accumulate(cam, env, W, H, k, DEPTH, rng, sum_, first=True)
        S.set_watertight(True)
        S.accumulate(cam, env, W, H, N - k, DEPTH, rng, sum_)
        checked = 0
        for px, py in ((0, 0), (W - 1, H - 1), (7, 9), (13, 4), (3, 12)):
            S.set_watertight(False)
            rgb_a, st_a = S.trace_pixel(cam, env, W, H, px, py, N, DEPTH)
            S.set_watertight(True)
            rgb_b, st_b = S.trace_pixel(cam, env, W, H, px, py, N, DEPTH)
            if st_a[k - 1] != st_b[k - 1]:
                continue
            checked += 1
            assert (_bits(sum_.reshape(-1, 3)[px + W * py]) == _bits(_fold(list(rgb_a[:k]) + list(rgb_b[k:])))).all(), (px, py)
            assert rng[px + W * py] == st_b[N - 1]
        assert checked >= 3, checked
    finally:
        S.set_watertight(False)


def test_refusals(orc, cornell, S):
    cam, env = _cam(orc, cornell), orc.make_env(**ENV)
    rng, sum_ = _fresh()
    with pytest.raises(RuntimeError):
        S.accumulate(cam, env, W, H, 0, DEPTH, rng, sum_, first=True)
    with pytest.raises(RuntimeError):
        S.accumulate(cam, env, W, H, 1, DEPTH, rng, sum_, pixel_list=[W * H], first=True)
    with pytest.raises(ValueError):
        S.accumulate(cam, env, W, H, 1, DEPTH, rng, sum_, pixel_list=[3, 3], first=True)
    with pytest.raises(ValueError):
        S.accumulate(cam, env, W, H, 1, DEPTH, rng[:-1], sum_, first=True)
    with pytest.raises(ValueError):
        S.accumulate(cam, env, W, H, 1, DEPTH, rng, sum_.astype(np.float64), first=True)
    assert (rng == 0xDEADBEEF).all() and (sum_ == F32(-7.25)).all(), "a refused call writes nothing"
