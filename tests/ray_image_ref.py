"""The oracle side of pt_render_rays (include/mi355pt.h "ray images"), for tests/test_ray_image_host.py and tests/test_gpu_ray_image.py.

The oracle has a ray generator for ray images, Scene.render_rays (orc_render_rays): orc_render's sample loop with the record's ray in the
camera's place, so a jittered frame of any size has an exact reference.  tests/test_ray_image_host.py anchors that generator before
anything is held to it, from two sides that do not use it:

* the degenerate camera.  A camera {origin = o, llc = L, horizontal = 0, vertical = 0} sends every sample of every pixel along
  normalize(((L + 0 * su) + 0 * sv) - o) = normalize(fl(L - o)) while pixel (x, y) keeps its own stream rng_init(x, y) and makes its two
  draws per sample.  So pixel (x, y) of a ray image with zero jitter is pixel (x, y) of Scene.render with the degenerate camera of its
  record, whenever the record's dir is fl(L - o): the tests choose o and L, never dir.  One Scene.render per ray with
  pixel_list = [id]; a call takes a tenth of a millisecond (oracle_pixels).  At W = H = 1 with org = 0 the record {0, dir, du, dv} is the
  camera {0, dir, du, dv} (oracle_jitter_1x1).
* the numpy restatement of a sample's first ray (first_sums here with form "right", normalised, and aov_rays_ref.table_rays, which it must equal):
  rng_init / rng_next and float32 numpy arithmetic only.  Behind the first ray there is one trace_path, which
  tests/test_oracle_vs_reference.py holds to the reference.  The other forms of first_sums are the mistakes a kernel could make; each
  must differ from the oracle."""
import numpy as np

F32 = np.float32


def degenerate_camera(o, L):
    """(the 12 floats of the camera {o, L, 0, 0}, the direction fl(L - o) of the ray it stands for) in float32."""
    o, L = np.asarray(o, F32).reshape(3), np.asarray(L, F32).reshape(3)
    return np.concatenate([o, L, np.zeros(6, F32)]).astype(F32), (L - o).astype(F32)


def rays_through(orgs, targets):
    """(orgs, dirs) of the rays from orgs towards the points `targets`, both (n, 3): dirs = fl(targets - orgs), what degenerate_camera
    reports for each pair."""
    o, L = np.ascontiguousarray(orgs, F32).reshape(-1, 3), np.ascontiguousarray(targets, F32).reshape(-1, 3)
    return o, (L - o).astype(F32)


def pixel_centre_targets(cam12, W, H):
    """The points on the image plane of the camera (12 floats) through which the pixel centres are seen, (W * H, 3) float32 in launch order
    x + W * y.  Any rounding will do: the ray is whatever fl(target - origin) turns out to be."""
    a = np.asarray(cam12, F32).reshape(12).astype(np.float64)
    x = (np.tile(np.arange(W), H) + 0.5)[:, None] / W
    y = (np.repeat(np.arange(H), W) + 0.5)[:, None] / H
    return (a[3:6] + a[6:9] * x + a[9:12] * y).astype(F32)


def oracle_pixels(orc, S, env, orgs, targets, W, H, spp, depth, ids=None, counters=None):
    """The oracle's frame of the ray image {org = orgs[id], dir = fl(targets[id] - orgs[id]), du = dv = 0}: ((H, W, 3) float32, (H, W)
    uint32) in framebuffer order, the pixels of `ids` (launch ids x + W * y; None: all) filled in and the rest +0.  counters: a dict
    the pixels' counters are added to."""
    o, L = np.ascontiguousarray(orgs, F32).reshape(-1, 3), np.ascontiguousarray(targets, F32).reshape(-1, 3)
    assert o.shape == (W * H, 3) and L.shape == (W * H, 3)
    rgb, rgba = np.zeros((H, W, 3), F32), np.zeros((H, W), np.uint32)
    one = np.zeros((H, W, 3), F32)
    for i in (range(W * H) if ids is None else ids):
        i = int(i)
        cam, _ = degenerate_camera(o[i], L[i])
        _, one8, cnt = S.render(orc.camera_from_array(cam), env, W, H, spp, depth, pixel_list=[i], want_rgba8=True, threads=1, out=one,
                                want_counters=counters is not None)
        if counters is not None:
            for k, v in cnt.items():
                counters[k] = counters.get(k, 0) + v
        x, y = i % W, i // W
        rgb[H - 1 - y, x] = one[H - 1 - y, x]
        rgba[H - 1 - y, x] = one8[H - 1 - y, x]
        one[H - 1 - y, x] = 0.0
    return rgb, rgba


def oracle_jitter_1x1(orc, S, env, d, du, dv, spp, depth):
    """The oracle's 1 x 1 frame of the record {org = 0, dir = d, du, dv}: Scene.render of the camera {0, d, du, dv} ((3,) float32, uint32)."""
    cam = np.concatenate([np.zeros(3, F32), np.asarray(d, F32), np.asarray(du, F32), np.asarray(dv, F32)]).astype(F32)
    rgb, rgba, _ = S.render(orc.camera_from_array(cam), env, 1, 1, spp, depth, want_rgba8=True, threads=1)
    return rgb[0, 0], rgba[0, 0]


FORMS = {"right": "normalize((dir + du * rx) + dv * ry)", "neighbour": "du and dv of the record in front (the last record's for record 0)",
         "swapped": "normalize((dir + du * ry) + dv * rx)", "dv_first": "normalize((dir + dv * ry) + du * rx)"}


def draws(orc, W, H, n_samples):
    """(rx, ry), each (W * H, n_samples) float32: the first two draws of every sample of every pixel's stream, as far as the first ray
    goes - sample k > 0 of a real path starts where sample k - 1 ended, so only column 0 is a frame's; the columns behind it are the
    draws 2k and 2k + 1 of the stream, what aov_rays_ref.table_rays uses."""
    rx, ry = np.zeros((W * H, n_samples), F32), np.zeros((W * H, n_samples), F32)
    for i in range(W * H):
        st = orc.rng_init(i % W, i // W)
        for k in range(n_samples):
            rx[i, k], st = orc.rng_next(st)
            ry[i, k], st = orc.rng_next(st)
    return rx, ry


def first_sums(table, rx, ry, form="right"):
    """The unnormalised float32 direction of a sample of every record (n, 3) for draws rx, ry (n,), one IEEE operation per numpy
    operation, in one of FORMS."""
    table = np.asarray(table).reshape(-1)
    d, du, dv = (np.ascontiguousarray(table[f], F32) for f in ("dir", "du", "dv"))
    rx, ry = np.asarray(rx, F32)[:, None], np.asarray(ry, F32)[:, None]
    if form == "right":
        return ((d + du * rx) + dv * ry).astype(F32)
    if form == "neighbour":
        return ((d + np.roll(du, 1, axis=0) * rx) + np.roll(dv, 1, axis=0) * ry).astype(F32)
    if form == "swapped":
        return ((d + du * ry) + dv * rx).astype(F32)
    if form == "dv_first":
        return ((d + dv * ry) + du * rx).astype(F32)
    raise KeyError(form)


def one_sample_table(table, rx0, ry0, form="right"):
    """The zero-jitter table {org, s, 0, 0} with s = first_sums of sample 0: its 1 spp frame is the 1 spp frame of `table` under a generator
    of the given form, because (s + 0 * rx) + 0 * ry = s and the two draws are made whatever the jitter is."""
    t = np.asarray(table).reshape(-1).copy()
    t["dir"] = first_sums(table, rx0, ry0, form)
    t["du"] = 0.0
    t["dv"] = 0.0
    return t
