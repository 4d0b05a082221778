"""What tests/test_gpu_queue.py and tests/test_queue_host.py share: the seeded cost images that the GPU cases inject with
pt_debug_set_cost_image, and the table of those cases (size, shard, image, cost_radius, options).  No GPU is needed to build any of it:
the host test shows on the same images that each wrong variant of tests/queue_ref.py differs from the right definition."""
import numpy as np

from owl_path_tracer_amd.pyhost import binding as B

SORT_BLOCK = 256 * 16  # PT_SORT_BLOCK * PT_SORT_ITEMS: queue entries per workgroup of the sort kernels
CLAMP_VALUES = (1, 105, 106, 107, 226, 227, 230, 231, 255)  # around both clamps of cost_bucket: class >= 227 is bucket 0, class <= 106 bucket 31
FLAT_CLASS = 150
CHEAP_CLASS, DEAR_CLASSES = 130, (180, 200)  # bucket 25 against buckets 12 .. 7


def stripes(W, H):
    """(i): every bucket 0 .. 31 in horizontal stripes of class 230 - 4 b + (x % 4); neighbouring stripes are 4 classes apart, so a
    de-noising window that crosses stripes meets classes up to +-11 from the pixel's own: both sides of the +-10 band."""
    s = max(1, H // 32)
    y, x = np.mgrid[0:H, 0:W]
    return (230 - 4 * ((y // s) % 32) + (x % 4)).astype(np.uint8)


def clamp_values(W, H, seed):
    """(iii): uniform over CLAMP_VALUES."""
    return np.random.default_rng(seed).choice(np.array(CLAMP_VALUES, np.uint8), size=(H, W))


def tail(W, H, seed):
    """(iv): one cheap class, and 2 % of the pixels (the fewest 5 x 5 blobs that reach W * H / 50) in classes at least 12 buckets dearer."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), CHEAP_CLASS, np.uint8)
    while (img != CHEAP_CLASS).sum() * 50 < W * H:
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        blob = img[y:y + 5, x:x + 5]
        blob[...] = rng.integers(DEAR_CLASSES[0], DEAR_CLASSES[1] + 1, blob.shape)
    return img


def flat(W, H):
    """(v)"""
    return np.full((H, W), FLAT_CLASS, np.uint8)


def case(name, W, H, kind, R, n, whole=-1, bpc=0, shard=None, frames=1):
    return dict(name=name, W=W, H=H, kind=kind, R=R, n=n, whole=whole, bpc=bpc, shard=shard, frames=frames)


SHARD = (1, 2, 16)  # (vi): rank 1 of 2, tiles of 16

# Queue lengths: 1; the last full sort block and the first ragged one (4 095, 4 096, 4 097); three blocks (8 193); eight and nine blocks
# (32 768, 32 769: the scan's `per` goes from 1 to 2 at 9 * 32 = 288 > 256 entries); eighteen blocks (71 033).
CASES = [case("len-%d" % (w * h), w, h, "stripes", 2, w * h) for w, h in ((1, 1), (65, 63), (64, 64), (3, 2731), (256, 128), (283, 251))]
for _w, _h, _n in ((17, 241, 4097), (99, 331, 32769)):
    for _R in (0, 2, 5):
        CASES.append(case("stripes-%d-R%d" % (_n, _R), _w, _h, "stripes", _R, _n))
        CASES.append(case("clamp-%d-R%d" % (_n, _R), _w, _h, "clamp", _R, _n))
for _w, _h, _n in ((23, 359, 4097), (853, 77, 32769)):  # rank 1 of 2 owns exactly this many pixels of such a frame
    for _R in (0, 2, 5):
        CASES.append(case("shard-%d-R%d" % (_n, _R), _w, _h, "stripes", _R, _n, shard=SHARD))
CASES.append(case("batch-3x61x47", 61, 47, "stripes", 2, 3 * 61 * 47, frames=3))
# the tier plan and its consumption
CASES.append(case("forced-32-tiers", 64, 48, "stripes", 0, 64 * 48, whole=1))
CASES.append(case("forced-clamp", 64, 48, "clamp", 2, 64 * 48, whole=1))
CASES.append(case("auto-tail", 96, 64, "tail", 2, 96 * 64, bpc=1))
CASES.append(case("auto-flat", 96, 64, "flat", 2, 96 * 64, bpc=1))
# (of the sizes above the smallest whose forced plan has fewer path slots than pixels with one workgroup per CU on 256 CUs: pt_debug_plan_tiers
# gives 8 758 slots for these 32 768 pixels, and 8 220 slots for the 8 193 pixels of 3 x 2731; the test asserts the inequality)
CASES.append(case("forced-tail-rounds", 256, 128, "tail", 2, 256 * 128, whole=1, bpc=1))
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def input_ids(c):
    """The input queue of the case's launch sequence: the shard's pixels in tile order (pt_shard_pixels), of a batch once per frame with the
    ids moved down by the frames above (the virtual image W x K*H)."""
    rank, world, tile = c["shard"] or (0, 1, 16)
    one = B.shard_pixels(c["W"], c["H"], tile, rank, world).astype(np.uint32)
    return np.concatenate([one + np.uint32(f * c["W"] * c["H"]) for f in range(c["frames"])])


def cost_image(c):
    """The image the case injects: (frames * H, W) uint8; with a shard, 0 at the pixels the rank does not own."""
    W, Hv = c["W"], c["H"] * c["frames"]
    seed = [W, Hv, c["R"]]
    img = {"stripes": lambda: stripes(W, Hv), "clamp": lambda: clamp_values(W, Hv, seed), "tail": lambda: tail(W, Hv, seed), "flat": lambda: flat(W, Hv)}[c["kind"]]()
    if c["shard"]:
        own = np.zeros(W * Hv, bool)
        own[input_ids(c)] = True
        img = np.where(own.reshape(Hv, W), img, 0).astype(np.uint8)
    return img
