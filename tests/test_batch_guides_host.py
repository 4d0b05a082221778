"""The batch forms of the guide pass and the denoiser (pt_render_aov_batch, pt_denoise_batch) without a GPU.

* The four exports exist, are in B.EXPORTS and in the header; the ABI version is still 5.
* On a host-only context every refusal of the header returns PT_E_INVALID with the call's name in pt_last_error, valid arguments return
  PT_E_NO_DEVICE, and output buffers pre-filled with 7 stay 7.
* `make asm-aov-follow-batch`: exactly three kernels, each a pt_aov_follow_batch instance, no scratch, at most 128 VGPRs (the budget of
  the four waves per SIMD the guide instances are built for); `make asm-denoise-batch`: exactly three kernels, no scratch.
* The references tests/test_gpu_batch_guides.py uses are sound on the CPU: for every frame of batch_guides_common.py - the moved cameras,
  the changed tables - pt_debug_aov_follow_host equals tests/aov_follow_ref.py over a `flat` built with the frame's table."""
import ctypes as C
import re

import numpy as np
import pytest

import batch_guides_common as BG
import resource_report
from owl_path_tracer_amd.pyhost import binding as B

F32 = np.float32
PT_E_INVALID, PT_E_NO_DEVICE, PT_E_NO_SCENE = -1, -2, -4
NAMES = ("pt_render_aov_batch", "pt_render_aov_batch_device", "pt_denoise_batch", "pt_denoise_batch_device")
fp = C.POINTER(C.c_float)


def test_exports_and_abi():
    L = B.lib()
    header = open(B.HEADER_PATH).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in B.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert L.pt_abi_version() == 5
    listed = re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)
    assert "pt_render_aov_batch_device" in listed and "pt_denoise_batch_device" in listed


def _refused(ctx, rc, who):
    assert rc == PT_E_INVALID, (who, rc)
    msg = B.lib().pt_last_error(ctx._h).decode()
    assert who in msg, (who, msg)
    return msg


def test_guide_batch_refusals_on_a_host_only_context():
    L = B.lib()
    name, W, H = "mirror_wall", 8, 8
    sc = BG.scene(name)
    n_mat = len(sc["mats"])
    arr, n, keep = B._marshal_frames(BG.frames(name, W, H, B))
    assert n == n_mat
    out = np.full((3, H, W, 8), 7.0, F32)
    outp = out.ctypes.data_as(fp)
    ok = B.aov_default_params()
    ctx = B.Context(-1)
    try:
        assert L.pt_render_aov_batch(ctx._h, arr, 3, n_mat, W, H, None, outp) == PT_E_NO_SCENE
        BG.upload(ctx, sc, B)

        def both(check, frames=arr, k=3, nm=n_mat, w=W, h=H, p=None):
            pp = C.byref(p) if p is not None else None
            check(L.pt_render_aov_batch(ctx._h, frames, k, nm, w, h, pp, outp), "pt_render_aov_batch")
            check(L.pt_render_aov_batch_device(ctx._h, frames, k, nm, w, h, pp, C.c_void_p(16), None), "pt_render_aov_batch_device")

        refused = lambda rc, who: _refused(ctx, rc, who)
        both(refused, k=0)
        both(refused, k=-1)
        both(refused, frames=None)
        both(refused, nm=n_mat + 1)
        both(refused, nm=0)
        for w, h in ((0, 8), (8, -1), (65536, 8), (8, 65536)):
            both(refused, w=w, h=h)
        for bad in (dict(n_samples=0), dict(max_follow=-1), dict(max_follow=9), dict(roughness_max=-0.01), dict(roughness_max=1.01), dict(roughness_max=float("nan")),
                    dict(reserved=1)):
            both(refused, p=B.aov_default_params(**bad))
        ctx.set_option("watertight", 1)
        both(lambda rc, who: "watertight" in _refused(ctx, rc, who) or pytest.fail("the refusal must name the option"))
        ctx.set_option("watertight", 0)
        assert L.pt_render_aov_batch(None, arr, 3, n_mat, W, H, None, outp) == PT_E_INVALID
        _refused(ctx, L.pt_render_aov_batch(ctx._h, arr, 3, n_mat, W, H, None, None), "pt_render_aov_batch")
        _refused(ctx, L.pt_render_aov_batch_device(ctx._h, arr, 3, n_mat, W, H, None, None, None), "pt_render_aov_batch_device")
        # valid arguments: no CPU fallback of the render entry points
        both(lambda rc, who: rc == PT_E_NO_DEVICE or pytest.fail("%s: %d" % (who, rc)))
        both(lambda rc, who: rc == PT_E_NO_DEVICE or pytest.fail("%s: %d" % (who, rc)), p=ok)
        both(lambda rc, who: rc == PT_E_NO_DEVICE or pytest.fail("%s: %d" % (who, rc)), k=1, p=B.aov_default_params(max_follow=0))
        assert (out == 7.0).all(), "a refused call wrote to the output"
    finally:
        ctx.close()
    del keep


def test_denoise_batch_refusals_on_a_host_only_context():
    L = B.lib()
    K, W, H = 3, 5, 4
    rgb = np.full((K, H, W, 3), 7.0, F32)
    aov = np.full((K, H, W, 8), 7.0, F32)
    out = np.full((K, H, W, 3), 7.0, F32)
    out8 = np.full((K, H, W), 7, np.uint32)
    rp, ap, op, o8 = rgb.ctypes.data_as(fp), aov.ctypes.data_as(fp), out.ctypes.data_as(fp), out8.ctypes.data_as(C.POINTER(C.c_uint32))
    d = C.c_void_p(16)
    ctx = B.Context(-1)  # no scene is needed
    try:
        def both(check, k=K, w=W, h=H, p=None):
            pp = C.byref(p) if p is not None else None
            check(L.pt_denoise_batch(ctx._h, rp, ap, k, w, h, pp, op, o8), "pt_denoise_batch")
            check(L.pt_denoise_batch_device(ctx._h, d, d, k, w, h, pp, d, d, None), "pt_denoise_batch_device")

        refused = lambda rc, who: _refused(ctx, rc, who)
        both(refused, k=0)
        both(refused, k=-2)
        for w, h in ((0, 4), (5, 0), (65536, 4), (5, 65536)):
            both(refused, w=w, h=h)
        for bad in (dict(iterations=0), dict(iterations=9), dict(flags=2), dict(sigma_color=0.0), dict(sigma_normal=-1.0), dict(sigma_depth=float("nan")),
                    dict(sigma_albedo=0.0)):
            both(refused, p=B.denoise_default_params(**bad))
        for args in ((None, ap, K, W, H, None, op, o8), (rp, None, K, W, H, None, op, o8), (rp, ap, K, W, H, None, None, o8)):
            _refused(ctx, L.pt_denoise_batch(ctx._h, *args), "pt_denoise_batch")
        for args in ((None, d, K, W, H, None, d, d, None), (d, None, K, W, H, None, d, d, None), (d, d, K, W, H, None, None, d, None)):
            _refused(ctx, L.pt_denoise_batch_device(ctx._h, *args), "pt_denoise_batch_device")
        assert L.pt_denoise_batch(None, rp, ap, K, W, H, None, op, o8) == PT_E_INVALID
        no_device = lambda rc, who: rc == PT_E_NO_DEVICE or pytest.fail("%s: %d" % (who, rc))
        both(no_device)
        both(no_device, p=B.denoise_default_params(iterations=8, flags=1, sigma_depth=float("inf")))
        both(no_device, k=1)
        assert L.pt_denoise_batch(ctx._h, rp, ap, K, W, H, None, op, None) == PT_E_NO_DEVICE  # out_rgba8 is optional
        assert L.pt_denoise_batch(ctx._h, rp, ap, K, W, H, None, rp, None) == PT_E_NO_DEVICE  # out_rgb may equal rgb
        assert (out == 7.0).all() and (out8 == 7).all() and (rgb == 7.0).all(), "a refused call wrote to a buffer"
    finally:
        ctx.close()


def test_batch_guide_kernels_need_no_scratch_and_fit_128_vgprs():
    blocks = resource_report.report("asm-aov-follow-batch")[1]
    names = [b[0] for b in blocks]
    assert len(blocks) == 3 and len(set(names)) == 3, names  # the binary walk and the two slab forms of the quad walk
    assert all("pt_aov_follow_batch" in nm for nm in names), names
    for nm, vgprs, scratch in blocks:
        assert int(scratch) == 0 and 0 < int(vgprs) <= 128, (nm, vgprs, scratch)


def test_batch_denoise_kernels_need_no_scratch():
    blocks = resource_report.report("asm-denoise-batch")[1]
    names = [b[0] for b in blocks]
    assert len(blocks) == 3 and len(set(names)) == 3, names
    for stage in ("prepare", "iter", "finish"):
        assert sum("pt_denoise_batch_%s_kernel" % stage in nm for nm in names) == 1, names
    assert all(int(scratch) == 0 for _, _, scratch in blocks), blocks


@pytest.mark.parametrize("W,H,n", [(37, 23, 3), (24, 16, 1)])
@pytest.mark.parametrize("name", sorted(BG.FRAMES))
def test_the_twin_of_every_frame_equals_the_restatement(orc, name, W, H, n):
    for frame in BG.FRAMES[name]:
        for k in (0, 4):
            want = BG.reference(orc, name, frame, W, H, n, k, 0.3)
            assert np.isfinite(want).all()
            BG.assert_same(BG.twin(B, name, frame, W, H, n, k, 0.3), want, "%s camera %d table %s %dx%d n=%d max_follow=%d: host twin vs aov_follow_ref" % ((name,) + frame + (W, H, n, k)))
    # the frames differ: another camera or another table shows in the bits
    a = [BG.twin(B, name, f, W, H, n, 4, 0.3) for f in BG.FRAMES[name]]
    assert (BG.bits(a[0]) != BG.bits(a[1])).any() and (BG.bits(a[1]) != BG.bits(a[2])).any() and (BG.bits(a[0]) != BG.bits(a[2])).any()
