"""The oracle side of pt_render_rays (include/mi355pt.h "ray images"), for tests/test_ray_image_host.py and tests/test_gpu_ray_image.py.

The oracle knows cameras only, and that is enough: a camera {origin = o, llc = L, horizontal = 0, vertical = 0} sends every sample of
every pixel along normalize(((L + 0 * su) + 0 * sv) - o) = normalize(fl(L - o)) while pixel (x, y) keeps its own stream rng_init(x, y)
and makes its two draws per sample.  So pixel (x, y) of a ray image with zero jitter is pixel (x, y) of Scene.render with the degenerate
camera of its record, whenever the record's dir is fl(L - o): the tests choose o and L, never dir.  One Scene.render per ray with
pixel_list = [id]; a call takes a tenth of a millisecond.

The jitter identity needs no trick: at W = H = 1 with org = 0 the record {0, dir, du, dv} is the camera {0, dir, du, dv}."""
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


def oracle_pixels(orc, S, env, orgs, targets, W, H, spp, depth, ids=None):
    """The oracle's frame of the ray image {org = orgs[id], dir = fl(targets[id] - orgs[id]), du = dv = 0}: ((H, W, 3) float32, (H, W)
    uint32) in framebuffer order, the pixels of `ids` (launch ids x + W * y; None: all) filled in and the rest +0."""
    o, L = np.ascontiguousarray(orgs, F32).reshape(-1, 3), np.ascontiguousarray(targets, F32).reshape(-1, 3)
    assert o.shape == (W * H, 3) and L.shape == (W * H, 3)
    rgb, rgba = np.zeros((H, W, 3), F32), np.zeros((H, W), np.uint32)
    one = np.zeros((H, W, 3), F32)
    for i in (range(W * H) if ids is None else ids):
        i = int(i)
        cam, _ = degenerate_camera(o[i], L[i])
        _, one8, _ = S.render(orc.camera_from_array(cam), env, W, H, spp, depth, pixel_list=[i], want_rgba8=True, threads=1, out=one)
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
