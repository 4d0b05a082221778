"""The cost-ordered pixel queue of csrc/pt_schedule.hip in numpy, in one place: the de-noised cost class of a pixel (pixel_cost), its
bucket (cost_bucket), and the stable counting sort of a launch's queue by that bucket (pt_sort_hist / _scan / _scatter_kernel).

Written from the text of pt_schedule.hip:
  * the (2R+1)^2 window of a pixel is clipped at the image;
  * a neighbour (the pixel itself included) counts if its class is != 0 and within +-10 classes of the pixel's own;
  * the estimate is the CEILING mean of the classes that count, the pixel's own class if none does, and never below the pixel's own;
  * the bucket is (230 - class) / 4 with C truncation, clamped to 0 .. 31 (0 = most expensive);
  * the queue is the input queue in non-decreasing bucket order, input order kept within a bucket.

Two forms: the vectorised one the GPU tests use, and a plain per-pixel loop (pixel_cost_loop, cost_bucket_loop, queue_ref_loop) that only
exists to check the vectorised one on the CPU (tests/test_queue_host.py).  VARIANTS names five deliberately WRONG definitions; the tests
show that the GPU cases can tell each of them from the right one."""
import numpy as np

BUCKETS = 32   # PT_SORT_BUCKETS
COST_TOP = 230 # PT_COST_TOP
BAND = 10      # PT_COST_BAND

# The wrong definitions: the band 9 classes wide; the floor mean; zeros inside the clipped window (pixels of another rank) take part in
# the mean as class 0; the window wrapped round the image, not clipped; input order reversed within a bucket.
# ("zeros_count" lets EVERY zero of the window count.  Dropping only the kernel's `v != 0` and keeping the band can never show in a queue:
# 0 is within +-10 of classes 0 .. 10 alone, the estimate of such a pixel is at most 20 either way, and every class up to 106 is bucket
# 31 - tests/test_queue_host.py::test_zero_inside_the_band_cannot_move_a_bucket.)
VARIANTS = ("band9", "floor_mean", "zeros_count", "wrap", "unstable")


def cost_bucket(cls):
    """cost_bucket() for an integer array of classes: (230 - cls) / 4 truncated toward zero as C does, clamped to 0 .. 31."""
    d = COST_TOP - np.asarray(cls, np.int64)
    return np.clip(np.sign(d) * (np.abs(d) // 4), 0, BUCKETS - 1)


def pixel_classes(img, R, variant=None):
    """pixel_cost() of every pixel of the cost image img (H, W): the de-noised class, as an (H, W) int64 array."""
    assert variant is None or variant in VARIANTS
    img = np.asarray(img).astype(np.int64)
    H, W = img.shape
    band = 9 if variant == "band9" else BAND
    if variant == "wrap":
        pad = np.pad(img, R, mode="wrap") if R else img
        inside = np.ones_like(pad, bool)
    else:
        pad = np.pad(img, R)
        inside = np.pad(np.ones_like(img, bool), R)
    total = np.zeros((H, W), np.int64)
    cnt = np.zeros((H, W), np.int64)
    for dy in range(2 * R + 1):
        for dx in range(2 * R + 1):
            v = pad[dy:dy + H, dx:dx + W]
            ok = (np.abs(v - img) <= band) & (v != 0)
            if variant == "zeros_count":
                ok |= v == 0
            ok &= inside[dy:dy + H, dx:dx + W]
            total += np.where(ok, v, 0)
            cnt += ok
    safe = np.maximum(cnt, 1)
    mean = total // safe if variant == "floor_mean" else (total + cnt - 1) // safe
    return np.maximum(img, np.where(cnt > 0, mean, img))


def queue_ref(ids, cost_img, W, H, R, variant=None):
    """The queue the device must build from the input queue `ids` (pixel ids x + W * y) and the cost image (H, W): returns
    (ids in stable bucket order, the 32-bin histogram of the entries' buckets)."""
    ids = np.asarray(ids)
    img = np.asarray(cost_img).reshape(H, W)
    bucket = cost_bucket(pixel_classes(img, R, variant).reshape(-1)[ids])
    hist = np.bincount(bucket, minlength=BUCKETS).astype(np.uint32)
    if variant == "unstable":  # input order reversed within a bucket
        order = np.argsort(bucket[::-1], kind="stable")
        return ids[::-1][order], hist
    return ids[np.argsort(bucket, kind="stable")], hist


def _queue_classes(ids, cost, q, W, H, R=2):
    """cost_bucket(pixel_cost()) for the queue entries q, from the cost per input entry as pt_debug_read_queue returns it: the pre-pass class
    of a pixel (16 per doubling of the time its pre-pass samples took), replaced by the mean over the neighbours within +-10 classes if
    that is larger, in buckets of 4 from 230 down.  Pixels that are in no entry hold 0."""
    img = np.zeros((H, W), np.int64)
    img.reshape(-1)[ids] = cost
    return cost_bucket(pixel_classes(img, R).reshape(-1)[q])


# ---- the same definition, pixel by pixel in plain Python -----------------------------------------------------------------------------

def pixel_cost_loop(img, x, y, R):
    H, W = len(img), len(img[0])
    own = int(img[y][x])
    total = cnt = 0
    for dy in range(-R, R + 1):
        yy = y + dy
        if yy < 0 or yy >= H:
            continue
        for dx in range(-R, R + 1):
            xx = x + dx
            if xx < 0 or xx >= W:
                continue
            v = int(img[yy][xx])
            if v != 0 and own - BAND <= v <= own + BAND:
                total += v
                cnt += 1
    mean = -((-total) // cnt) if cnt else own  # ceiling
    return mean if mean > own else own


def cost_bucket_loop(cls):
    d = COST_TOP - int(cls)
    b = d // 4 if d >= 0 else -((-d) // 4)  # C division truncates
    return 0 if b < 0 else (BUCKETS - 1 if b > BUCKETS - 1 else b)


def queue_ref_loop(ids, cost_img, W, H, R):
    img = [[int(v) for v in row] for row in np.asarray(cost_img).reshape(H, W)]
    lists = [[] for _ in range(BUCKETS)]
    for i in ids:
        i = int(i)
        lists[cost_bucket_loop(pixel_cost_loop(img, i % W, i // W, R))].append(i)
    return np.array([i for l in lists for i in l], np.uint32), np.array([len(l) for l in lists], np.uint32)
