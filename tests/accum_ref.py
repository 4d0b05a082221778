"""numpy restatement of the progressive accumulation's resolve and select (include/mi355pt.h, "progressive accumulation"), written from the
header text alone: float32 throughout, one rounding per written operation (numpy's float32 +, -, *, / and sqrt are correctly rounded),
max_ and make_rgba as csrc/pt_device.h defines them.  Works on arrays of any leading shape; colours have a last axis of 3."""
import numpy as np

F32 = np.float32
U32 = np.uint32
INF = F32(np.inf)


def max_(a, b):
    """pt_device.h max_: (b != b || a > b) ? a : b"""
    a, b = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32))
    return np.where((b != b) | (a > b), a, b).astype(F32)


def make_rgba(c):
    """pt_device.h make_rgba: min(255, max(0, int(f * 256))) per channel (NaN -> 0), alpha 255"""
    s = (np.asarray(c, F32) * F32(256.0)).astype(F32)
    s = np.where(s != s, F32(0.0), s)
    q = np.clip(np.trunc(np.clip(s.astype(np.float64), -2147483647.0, 2147483647.0)), 0, 255).astype(U32)
    return (q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | U32(0xFF000000)).astype(U32)


def resolve(sum_, seen, half, n, n_half, passes, active, owned, n_samples):
    """-> dict(seen, half, n, n_half, passes, rgb, rgba8, noise); the inputs are not changed."""
    sum_ = np.asarray(sum_, F32)
    seen, half = np.array(seen, F32), np.array(half, F32)
    n, n_half, passes = np.array(n, U32), np.array(n_half, U32), np.array(passes, U32)
    own = np.asarray(owned) != 0
    act = (np.asarray(active) != 0) & own
    odd = act & ((passes & U32(1)) == 1)
    with np.errstate(all="ignore"):
        half = np.where(odd[..., None], (half + (sum_ - seen).astype(F32)).astype(F32), half)
        n_half = np.where(odd, n_half + U32(n_samples), n_half).astype(U32)
        seen = np.where(act[..., None], sum_, seen)
        n = np.where(act, n + U32(n_samples), n).astype(U32)
        passes = np.where(act, passes + U32(1), passes).astype(U32)
        has = own & (n >= 1)
        inv = (F32(1.0) / n.astype(F32)).astype(F32)
        out = np.where(has[..., None], (sum_ * inv[..., None]).astype(F32), F32(0.0)).astype(F32)
        rgba8 = np.where(has, make_rgba(out), U32(0)).astype(U32)
        ia = (F32(1.0) / n_half.astype(F32)).astype(F32)
        ib = (F32(1.0) / (n - n_half).astype(U32).astype(F32)).astype(F32)
        a = (half * ia[..., None]).astype(F32)
        b = ((sum_ - half).astype(F32) * ib[..., None]).astype(F32)
        dk = np.abs((a - b).astype(F32))
        d = ((dk[..., 0] + dk[..., 1]).astype(F32) + dk[..., 2]).astype(F32)
        l = max_(((out[..., 0] + out[..., 1]).astype(F32) + out[..., 2]).astype(F32), F32(1e-2))
        noise = (d / np.sqrt(l).astype(F32)).astype(F32)
    noise = np.where(n_half == 0, INF, noise)
    noise = np.where(own, noise, F32(0.0)).astype(F32)
    return dict(seen=seen, half=half, n=n, n_half=n_half, passes=passes, rgb=out, rgba8=rgba8, noise=noise)


def select(noise, n, owned, max_pixel_samples=0, noise_threshold=0.0):
    """-> active flags (uint8): owned, under the cap, and !(noise <= threshold) when there is a threshold."""
    noise, n = np.asarray(noise, F32), np.asarray(n, U32)
    thr = F32(noise_threshold)
    with np.errstate(invalid="ignore"):
        act = (np.asarray(owned) != 0) & ((max_pixel_samples == 0) | (n < U32(max_pixel_samples))) & ((thr == 0) | ~(noise <= thr))
    return act.astype(np.uint8)
