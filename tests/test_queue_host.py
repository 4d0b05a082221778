"""CPU checks around the cost-ordered pixel queue (no GPU needed):

* the vectorised numpy definition of tests/queue_ref.py equals its plain per-pixel loop restatement - classes, buckets, queue and
  histogram - on random images up to 23 x 17, cost_radius 0, 1, 2 and 5, classes from the whole range 0 .. 255 with the values around
  both clamps of cost_bucket forced in, on full frames and on shards with zeros at the pixels of the other rank;
* each of the five wrong variants of queue_ref gives another queue than the right definition on at least one of the cases of
  tests/test_gpu_queue.py (tests/queue_common.py), so a variant the GPU cases could not tell apart is noticed here, without a GPU;
* the cases have the queue lengths they are meant to have;
* pt_debug_set_cost_image is exported, in the header and in B.EXPORTS, the ABI version is still 5, and the call refuses a host-only
  context (PT_E_NO_DEVICE, with an image and with NULL) and a NULL context (PT_E_INVALID)."""
import ctypes as C
import re

import numpy as np
import pytest

import queue_common as QC
import queue_ref as QR
from owl_path_tracer_amd.pyhost import binding as B

FORCED = (0, 1, 105, 106, 107, 226, 227, 230, 231, 255)


def _random_image(rng, W, H, kind):
    if kind == 0:  # the whole range
        img = rng.integers(0, 256, (H, W))
    elif kind == 1:  # a narrow range: nearly every neighbour is within the band, the means decide
        img = rng.integers(100, 125, (H, W))
    else:  # around the clamps, with zeros
        img = rng.choice(np.array(FORCED), size=(H, W))
    flat = img.reshape(-1)
    k = min(flat.size, len(FORCED))
    flat[rng.choice(flat.size, k, replace=False)] = FORCED[:k]
    return img.astype(np.uint8)


def test_bucket_clamps():
    cls = np.arange(256)
    want = np.array([QR.cost_bucket_loop(c) for c in cls])
    np.testing.assert_array_equal(QR.cost_bucket(cls), want)
    assert [QR.cost_bucket_loop(c) for c in (0, 1, 105, 106, 107, 110, 226, 227, 230, 231, 255)] == [31, 31, 31, 31, 30, 30, 1, 0, 0, 0, 0]


@pytest.mark.parametrize("R", [0, 1, 2, 5])
def test_vectorised_reference_equals_the_loop(R):
    rng = np.random.default_rng(1000 + R)
    seen = set()
    for trial in range(24):
        W, H = ((23, 17), (1, 1), (1, 9), (7, 1), (2, 2))[trial] if trial < 5 else (int(rng.integers(1, 24)), int(rng.integers(1, 18)))
        img = _random_image(rng, W, H, trial % 3)
        seen.update(int(v) for v in np.unique(img))
        want_cls = np.array([[QR.pixel_cost_loop(img.tolist(), x, y, R) for x in range(W)] for y in range(H)])
        np.testing.assert_array_equal(QR.pixel_classes(img, R), want_cls, err_msg="classes, %dx%d R %d" % (W, H, R))
        for rank, world in ((0, 1), (1, 2), (0, 3)):
            ids = B.shard_pixels(W, H, 8, rank, world)
            shard = img.copy()
            if world > 1:  # zeros where the rank owns nothing, as the pre-pass leaves them
                own = np.zeros(W * H, bool)
                own[ids] = True
                shard = np.where(own.reshape(H, W), img, 0).astype(np.uint8)
            q, hist = QR.queue_ref(ids, shard, W, H, R)
            ql, hl = QR.queue_ref_loop(ids, shard, W, H, R)
            np.testing.assert_array_equal(q, ql, err_msg="queue, %dx%d R %d shard %d/%d" % (W, H, R, rank, world))
            np.testing.assert_array_equal(hist, hl)
            assert hist.sum() == ids.size
            cls = QR._queue_classes(ids, shard.reshape(-1)[ids], q, W, H, R)
            assert np.all(np.diff(cls) >= 0)
    assert seen.issuperset(FORCED)


def test_zero_inside_the_band_cannot_move_a_bucket():
    """Why variant "zeros_count" lets every zero count: the kernel's `v != 0` alone, with the band kept, decides no bucket.  A zero is
    within +-10 of classes 0 .. 10 only; the estimate of such a pixel is at most 20 with or without it, and classes <= 106 share bucket 31."""
    rng = np.random.default_rng(7)
    moved = 0
    for trial in range(40):
        W, H, R = int(rng.integers(1, 12)), int(rng.integers(1, 12)), int(rng.integers(0, 4))
        img = rng.integers(0, (14, 256)[trial % 2], (H, W))
        for y in range(H):
            for x in range(W):
                own = int(img[y, x])
                win = img[max(0, y - R):y + R + 1, max(0, x - R):x + R + 1].reshape(-1)
                near = win[np.abs(win - own) <= QR.BAND]  # zeros included
                loose = max(own, -(-int(near.sum()) // near.size))
                strict = QR.pixel_cost_loop(img.tolist(), x, y, R)
                moved += loose != strict
                assert QR.cost_bucket_loop(loose) == QR.cost_bucket_loop(strict)
    assert moved > 0, "the classes themselves must differ somewhere, or nothing was compared"


def test_cases_have_the_lengths_they_are_meant_to_have():
    lengths = set()
    for c in QC.CASES:
        ids = QC.input_ids(c)
        assert ids.size == c["n"], c["name"]
        assert np.unique(ids).size == ids.size and ids.max() < c["W"] * c["H"] * c["frames"]
        lengths.add(ids.size)
    B_ = QC.SORT_BLOCK
    assert {1, B_ - 1, B_, B_ + 1, 2 * B_ + 1, 8 * B_, 8 * B_ + 1}.issubset(lengths) and max(lengths) >= 70000
    assert any(c["shard"] and c["n"] == B_ + 1 for c in QC.CASES) and any(c["shard"] and c["n"] == 8 * B_ + 1 for c in QC.CASES)
    assert {c["R"] for c in QC.CASES} == {0, 2, 5}


def test_cost_images_are_what_they_are_meant_to_be():
    img = QC.cost_image(QC.BY_NAME["forced-32-tiers"])
    _, hist = QR.queue_ref(QC.input_ids(QC.BY_NAME["forced-32-tiers"]), img, 64, 48, 0)
    assert (hist > 0).all(), "stripes at 64x48, R = 0: every one of the 32 buckets"
    img = QC.cost_image(QC.BY_NAME["auto-tail"])
    dear = img != QC.CHEAP_CLASS
    assert 0.02 <= dear.mean() < 0.03 and img[dear].min() >= QC.DEAR_CLASSES[0]
    assert QR.cost_bucket(QC.CHEAP_CLASS) - QR.cost_bucket(QC.DEAR_CLASSES[0]) >= 12
    assert set(np.unique(QC.cost_image(QC.BY_NAME["clamp-4097-R2"]))) == set(QC.CLAMP_VALUES)
    sh = QC.BY_NAME["shard-4097-R2"]
    img = QC.cost_image(sh)
    assert (img != 0).sum() == sh["n"] and (img.reshape(-1)[QC.input_ids(sh)] != 0).all()


@pytest.fixture(scope="module")
def right_queues():
    out = {}
    for c in QC.CASES:
        ids, img = QC.input_ids(c), QC.cost_image(c)
        out[c["name"]] = (ids, img, QR.queue_ref(ids, img, c["W"], c["H"] * c["frames"], c["R"])[0])
    return out


@pytest.mark.parametrize("variant", QR.VARIANTS)
def test_each_wrong_variant_differs_on_a_gpu_case(variant, right_queues):
    differs = []
    for c in QC.CASES:
        ids, img, right = right_queues[c["name"]]
        wrong, _ = QR.queue_ref(ids, img, c["W"], c["H"] * c["frames"], c["R"], variant)
        if not np.array_equal(wrong, right):
            differs.append(c["name"])
    assert differs, "no case of tests/queue_common.py tells variant %r from the definition" % variant


def test_set_cost_image_export_and_refusals_without_a_gpu():
    PT_E_INVALID, PT_E_NO_DEVICE = -1, -2
    L = B.lib()
    header = re.sub(r"/\*.*?\*/", "", open(B.HEADER_PATH).read(), flags=re.S)
    assert re.search(r"\bint\s+pt_debug_set_cost_image\s*\(\s*pt_ctx\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*img\s*,\s*int32_t\s+width\s*,\s*int32_t\s+height\s*\)\s*;", header)
    assert "pt_debug_set_cost_image" in B.EXPORTS and hasattr(C.CDLL(B.LIB_PATH), "pt_debug_set_cost_image")
    assert L.pt_abi_version() == 5
    img = np.full((4, 6), 150, np.uint8)
    assert L.pt_debug_set_cost_image(None, img.ctypes.data_as(C.POINTER(C.c_uint8)), 6, 4) == PT_E_INVALID
    ctx = B.Context(-1)
    try:
        assert L.pt_debug_set_cost_image(ctx._h, img.ctypes.data_as(C.POINTER(C.c_uint8)), 6, 4) == PT_E_NO_DEVICE
        assert "needs the GPU" in L.pt_last_error(ctx._h).decode()
        assert L.pt_debug_set_cost_image(ctx._h, None, 0, 0) == PT_E_NO_DEVICE
        with pytest.raises(B.PtError, match="pt_debug_set_cost_image.*needs the GPU"):
            ctx.set_cost_image(img)
        with pytest.raises(B.PtError, match="needs the GPU"):
            ctx.set_cost_image(None)
    finally:
        ctx.close()
