"""Ray images for Context.render_rays (pt_render_rays; include/mi355pt.h "ray images"): tables of W * H pt_ray_gen records, the record of
pixel (x, y) at launch index x + W * y.  A sample of the pixel starts at `org` and runs along normalize((dir + du * rx) + dv * ry) with
the pixel's own draws rx, ry in [0, 1).  The frame comes back in framebuffer order (row H - 1 - y), as from render(); to_list undoes that.

Everything here is host-side numpy in float64, rounded to float32 once per stored value."""
import numpy as np

from .binding import RAY_GEN_DTYPE

DTYPE = RAY_GEN_DTYPE  # org, reserved0, dir, reserved1, du, reserved2, dv, reserved3: 64 bytes


def _table(W, H):
    if W < 1 or H < 1:
        raise ValueError("ray image: bad size %dx%d" % (W, H))
    return np.zeros(W * H, DTYPE)


def _v3(a, n, what):
    a = np.asarray(a, np.float64)
    if a.shape == (3,):
        a = np.broadcast_to(a, (n, 3))
    if a.shape != (n, 3):
        raise ValueError("ray image: %s has shape %s, wanted (%d, 3) or (3,)" % (what, a.shape, n))
    return a


def fixed(orgs, dirs, W, H):
    """One fixed ray per pixel (zero jitter: every sample of the pixel runs along normalize(dir); the draws are still made).  orgs, dirs:
    (W * H, 3) in launch order x + W * y, or one (3,) vector for all pixels."""
    t = _table(W, H)
    t["org"] = _v3(orgs, W * H, "orgs")
    t["dir"] = _v3(dirs, W * H, "dirs")
    return t


def pinhole(cam, W, H):
    """The ray image of a pinhole camera (binding.Camera or its 12 floats origin, llc, horizontal, vertical): dir is the ray through the
    pixel's lower corner, llc + horizontal * (x / W) + vertical * (y / H) - origin, du = horizontal / W, dv = vertical / H, so that
    dir + du * rx + dv * ry is the camera's ray at ((x + rx) / W, (y + ry) / H) up to the rounding of the three stored vectors."""
    a = np.asarray(cam.as_array() if hasattr(cam, "as_array") else cam, np.float32).reshape(12).astype(np.float64)
    o, llc, hor, ver = a[0:3], a[3:6], a[6:9], a[9:12]
    x = np.tile(np.arange(W, dtype=np.float64), H)[:, None]
    y = np.repeat(np.arange(H, dtype=np.float64), W)[:, None]
    t = _table(W, H)
    t["org"] = o
    t["dir"] = llc + hor * (x / W) + ver * (y / H) - o
    t["du"] = hor / W
    t["dv"] = ver / H
    return t


def equirect_direction(x, y, W, H, up=(0, 1, 0), forward=(0, 0, -1)):
    """The unit direction of the equirectangular image at the continuous pixel position (x, y), y counted upwards like the launch index:
    azimuth phi = 2 pi (x / W - 1/2) about `up` (0 = forward, positive towards right = forward x up), elevation theta = pi (y / H - 1/2):
        d = cos(theta) * (cos(phi) * f + sin(phi) * r) + sin(theta) * u
    with f = forward normalised, u = the part of up orthogonal to f, normalised, r = cross(f, u).  Float64; x, y broadcast."""
    f = np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    u = np.asarray(up, np.float64)
    u = u - f * np.dot(u, f)
    if not np.linalg.norm(u) > 0:
        raise ValueError("equirect: up is parallel to forward")
    u = u / np.linalg.norm(u)
    r = np.cross(f, u)
    phi = 2.0 * np.pi * (np.asarray(x, np.float64) / W - 0.5)
    theta = np.pi * (np.asarray(y, np.float64) / H - 0.5)
    ct = np.cos(theta)[..., None]
    return ct * (np.cos(phi)[..., None] * f + np.sin(phi)[..., None] * r) + np.sin(theta)[..., None] * u


def equirect(origin, W, H, up=(0, 1, 0), forward=(0, 0, -1)):
    """A full-sphere panorama from `origin`: one direction per pixel centre, c(x, y) = equirect_direction(x + 1/2, y + 1/2).  du and dv are
    the finite differences to the neighbouring pixel's centre, du = c(x + 1, y) - c(x, y) and dv = c(x, y + 1) - c(x, y), and dir is
    c - (du + dv) / 2: the draws rx = ry = 1/2 give the centre direction and the samples cover the pixel's solid angle around it."""
    x = np.tile(np.arange(W, dtype=np.float64), H) + 0.5
    y = np.repeat(np.arange(H, dtype=np.float64), W) + 0.5
    c = equirect_direction(x, y, W, H, up, forward)
    du = equirect_direction(x + 1.0, y, W, H, up, forward) - c
    dv = equirect_direction(x, y + 1.0, W, H, up, forward) - c
    t = _table(W, H)
    t["org"] = np.asarray(origin, np.float64).reshape(3)
    t["dir"] = c - 0.5 * (du + dv)
    t["du"] = du
    t["dv"] = dv
    return t


def to_list(out, W, H):
    """A frame of render_rays ((H, W, ...) in framebuffer order) as a list in the rays' order: entry x + W * y is pixel (x, y)."""
    out = np.asarray(out)
    if out.shape[:2] != (H, W):
        raise ValueError("to_list: frame of shape %s, wanted (%d, %d, ...)" % (out.shape, H, W))
    return np.ascontiguousarray(out[::-1]).reshape((W * H,) + out.shape[2:])
