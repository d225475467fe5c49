"""The image stabilisation kernels (csrc/warp.hip, csrc/warp_pixel.h) on the device: the reference's epochs of
tests/golden/g15_stabilise.npz through the four Python entry points, and both kernels at every boundary between two code paths: the
64-pixel block in which the warp forms its coordinates, the 256-thread block, one and several images per launch, 1, 3 and 4 channels,
an output size other than the input's, taps one pixel outside on every side, equal weights, W = 0 and W < 0, maps entirely outside,
the integer and the short clamp, every length of the distortion vector, a non-finite coordinate, and the refusals of the C entry points.

Bound: equality of bytes with the numpy restatement (tests/warp_oracle.py), for every pixel of every case. Derived, not measured: the
kernels and the restatement perform the same IEEE float64 operations in the same order with contraction off, float64 division is
correctly rounded on the device, the rounding to 1/32 pixel is to even on both sides, everything behind it is integer arithmetic, and
the library is built without a fast-math flag. The host build of the same text agrees with the restatement on the same case lists
(tests/test_stabilise_cpu.py); what only this file can show is a lost `#pragma clang fp contract(off)`: gfx950 has fused multiply-add.

Every output of a C ABI call lies between two guard bands of sentinel bytes in one allocation and is itself pre-filled; the bands must
come back untouched."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import warp_oracle as W  # noqa: E402

pytestmark = pytest.mark.gpu

N = 7
FRAME = (96, 144)
BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -74


@pytest.fixture(scope="module")
def g15():
    with np.load(W.GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


@pytest.fixture(scope="module")
def epochs(g15):
    """(reference camera, epoch cameras, images [7, 96, 144, 3]): computed once, never changed."""
    from icepy4d_amd.core import Camera
    g = g15
    ref = Camera(FRAME[1], FRAME[0], g["ref_K"], g["ref_dist"], extrinsics=g["ref_extrinsics"].copy())
    cams = [Camera(FRAME[1], FRAME[0], g[f"ep{e}_K"], g[f"ep{e}_dist"], extrinsics=g[f"ep{e}_extrinsics"].copy()) for e in range(N)]
    imgs = np.stack([W.image_pattern(*FRAME, 3, seed=e) for e in range(N)])
    imgs.setflags(write=False)
    return ref, cams, imgs


def p(t):
    from icepy4d_amd._lib import ptr
    return ptr(t)


def dev(eng, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(eng.device)          # a copy: the shared inputs are read-only


class Framed:
    """An output of `nbytes` between two bands of sentinel bytes, in one device allocation."""

    def __init__(self, eng, shape):
        import torch
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        host = np.full(2 * BAND + self.n, SENT, np.uint8)
        host[BAND:BAND + self.n] = FILL
        self.buf = torch.from_numpy(host).to(eng.device)
        self.ptr = self.buf.data_ptr() + BAND

    def result(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all(), (what, "a byte outside the output was written")
        return host[BAND:BAND + self.n].reshape(self.shape)


def run_warp(eng, src, minv, oh, ow, what):
    n, h, w, c = src.shape
    d_src, d_m = dev(eng, src), dev(eng, np.ascontiguousarray(minv, np.float64).reshape(n, 9))
    out = Framed(eng, (n, oh, ow, c))
    eng.ctx.call("im_warp_perspective", p(d_src), n, h, w, c, p(d_m), oh, ow, out.ptr, eng.stream_ptr())
    return out.result(what)


def run_undistort(eng, src, row, what):
    n, h, w, c = src.shape
    d_src, row = dev(eng, src), np.ascontiguousarray(row, np.float64)
    out = Framed(eng, src.shape)
    eng.ctx.call("im_undistort_image", p(d_src), n, h, w, c, row.ctypes.data, out.ptr, eng.stream_ptr())
    return out.result(what)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (what, got.shape, want.shape)
    diff = got != want
    assert not diff.any(), (what, f"{int(diff.sum())} of {diff.size} bytes differ, first at {tuple(int(v) for v in np.argwhere(diff)[0])}")


# ---- the fixture through the Python entry points ---------------------------------------------------------------------------------------
def test_g15_through_the_python_entry_points(g15, eng, epochs, tmp_path):
    import torch
    from icepy4d_amd import sfm
    from icepy4d_amd.utils import homography as hom
    ref, cams, imgs = epochs
    for e, cam in enumerate(cams):
        same(sfm.undistort_image(imgs[e], cam, engine=eng), g15["undistorted"][e], f"undistort_image, epoch {e}")
        same(hom.homography_warping(ref, cam, imgs[e], engine=eng), g15["warped"][e], f"homography_warping, epoch {e}")
        same(hom.homography_warping(ref, cam, imgs[e], undistort=True, engine=eng), g15["warped_undistorted"][e], f"with undistortion, epoch {e}")
    # device tensors in, device tensors out; a grey image without a channel axis keeps its shape
    d = dev(eng, imgs[2])
    out = hom.homography_warping(ref, cams[2], d, undistort=True, engine=eng)
    assert isinstance(out, torch.Tensor) and out.device == eng.device
    same(out.cpu().numpy(), g15["warped_undistorted"][2], "device tensor")
    grey = np.ascontiguousarray(imgs[3][:, :, 1])
    same(sfm.undistort_image(grey, cams[3], engine=eng), g15["undistorted"][3][:, :, 1], "grey image")
    same(sfm.undistort_image(dev(eng, grey), cams[3], engine=eng).cpu().numpy(), g15["undistorted"][3][:, :, 1], "grey device image")
    # out_path: written through PIL as given (a lossless format reads back the same bytes)
    from PIL import Image
    path = tmp_path / "sub" / "warped.png"
    out = hom.homography_warping(ref, cams[0], imgs[0], undistort=True, out_path=path, engine=eng)
    same(np.asarray(Image.open(path)), out, "out_path")
    same(out, g15["warped_undistorted"][0], "out_path result")


def test_stabilise_sequence_equals_the_per_image_calls(g15, eng, epochs, monkeypatch):
    import torch
    from icepy4d_amd.utils import homography as hom
    ref, cams, imgs = epochs
    for undistort, key in ((True, "warped_undistorted"), (False, "warped")):
        out = hom.stabilise_sequence(ref, cams, list(imgs), undistort=undistort, engine=eng)
        assert isinstance(out, torch.Tensor) and out.device == eng.device and tuple(out.shape) == (N,) + FRAME + (3,)
        same(out.cpu().numpy(), g15[key], f"list, undistort = {undistort}")
        per_image = np.stack([hom.homography_warping(ref, cams[e], imgs[e], undistort=undistort, engine=eng) for e in range(N)])
        same(out.cpu().numpy(), per_image, "the per-image calls")
    same(hom.stabilise_sequence(ref, cams, dev(eng, imgs), engine=eng, to_host=True), g15["warped_undistorted"], "device tensor, to_host")
    # chunks of three images (and a last one of one): the bound on the working buffers, runs of equal intrinsics inside a chunk
    monkeypatch.setattr(hom, "WORK_BYTES", 2 * 3 * imgs[0].size)
    same(hom.stabilise_sequence(ref, cams, list(imgs), engine=eng, to_host=True), g15["warped_undistorted"], "chunks of three")
    monkeypatch.setattr(hom, "WORK_BYTES", 1)
    same(hom.stabilise_sequence(ref, cams, dev(eng, imgs), engine=eng, to_host=True), g15["warped_undistorted"], "one image per chunk")
    # smoothed cameras go through like any others
    smooth = hom.smooth_camera_rotations(cams)
    want = np.stack([W.warp_perspective(W.undistort(imgs[e], c.K, c.dist), hom.homography(ref, c), (FRAME[1], FRAME[0])) for e, c in enumerate(smooth)])
    same(hom.stabilise_sequence(ref, smooth, list(imgs), engine=eng, to_host=True), want, "smoothed cameras")


# ---- the warp at every path boundary ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", W.WARP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_warp_shapes_channels_matrices(eng, shape):
    cases = W.warp_cases([shape])
    assert len(cases) == 3 * (len(W.all_inverses(*shape)) + 1)
    for case in cases:
        same(run_warp(eng, *case[1:], case[0]), W.warp_expected(case), case[0])


def test_warp_to_another_size(eng):
    cases = [c for c in W.warp_cases() if "->" in c[0]]
    assert len(cases) == 3 and all(c[3:] == (7, 200) and c[1].shape[:3] == (3, 5, 65) for c in cases)
    for case in cases:
        same(run_warp(eng, *case[1:], case[0]), W.warp_expected(case), case[0])


# ---- the undistortion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.undistort_cases(), ids=lambda c: c[0])
def test_undistort_cases(eng, case):
    for c, n in ((3, 1), (1, 2), (4, 1)):
        src, row = W.undistort_inputs(case, c, n)
        want = np.stack([W.undistort_row(s, row) for s in src])
        same(run_undistort(eng, src, row, case[0]), want, f"{case[0]}, c = {c}, n = {n}")
        if case[0].startswith("zero distortion"):
            same(want, src, case[0] + " is the identity")


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_the_code_and_write_nothing(eng):
    import torch
    lib, ctx, s = eng.ctx.lib, eng.ctx.h, eng.stream_ptr()
    n, h, w, c = 2, 5, 9, 3
    src = dev(eng, np.stack([W.image_pattern(h, w, c, seed=k) for k in range(n)]))
    minv = dev(eng, np.tile(np.eye(3).ravel(), (n, 1)))
    row = W.cam_row(*W.scaled_calib("cam1", w))
    big = torch.full((2 * n * h * w * c,), SENT, dtype=torch.uint8, device=eng.device)      # for the overlapping ranges
    out = Framed(eng, (n, h, w, c))
    ps, pm, pr, po = p(src), p(minv), row.ctypes.data, out.ptr

    def refused(rc, what):
        assert rc == REFUSED, (what, rc)
        msg = lib.im_last_error(ctx).decode()
        assert msg.startswith("im_undistort_image: ") or msg.startswith("im_warp_perspective: "), (what, msg)

    U = lambda *a: lib.im_undistort_image(ctx, *a, s)          # noqa: E731  (d_src, n, h, w, c, h_cam, d_dst)
    P = lambda *a: lib.im_warp_perspective(ctx, *a, s)         # noqa: E731  (d_src, n, h, w, c, d_minv, oh, ow, d_dst)
    refused(U(None, n, h, w, c, pr, po), "null source")
    refused(U(ps, n, h, w, c, None, po), "null camera")
    refused(U(ps, n, h, w, c, pr, None), "null destination")
    refused(P(None, n, h, w, c, pm, h, w, po), "null source")
    refused(P(ps, n, h, w, c, None, h, w, po), "null matrices")
    refused(P(ps, n, h, w, c, pm, h, w, None), "null destination")
    refused(U(ps, n, h, w, c, pr, ps), "in place")
    refused(P(ps, n, h, w, c, pm, h, w, ps), "in place")
    pb = big.data_ptr()
    nbytes = n * h * w * c
    refused(U(pb, n, h, w, c, pr, pb + nbytes - 1), "ranges share one byte")
    refused(U(pb + nbytes - 1, n, h, w, c, pr, pb), "ranges share one byte, destination first")
    refused(P(pb, n, h, w, c, pm, 1, 1, pb + nbytes - 1), "a small destination inside the source")
    refused(P(pb + 1, 1, 1, 1, 1, pm, h, w, pb), "a small source inside the destination")
    for bad_c in (0, 5, -1):
        refused(U(ps, n, h, w, bad_c, pr, po), f"channels = {bad_c}")
        refused(P(ps, n, h, w, bad_c, pm, h, w, po), f"channels = {bad_c}")
    for bad in (0, -1, 32767, 2 ** 31 - 1):
        refused(U(ps, n, bad, w, c, pr, po), f"h = {bad}")
        refused(U(ps, n, h, bad, c, pr, po), f"w = {bad}")
        refused(P(ps, n, bad, w, c, pm, h, w, po), f"h = {bad}")
        refused(P(ps, n, h, bad, c, pm, h, w, po), f"w = {bad}")
        refused(P(ps, n, h, w, c, pm, bad, w, po), f"oh = {bad}")
        refused(P(ps, n, h, w, c, pm, h, bad, po), f"ow = {bad}")
    for bad_n in (0, -1, 65536):
        refused(U(ps, bad_n, h, w, c, pr, po), f"n_images = {bad_n}")
        refused(P(ps, bad_n, h, w, c, pm, h, w, po), f"n_images = {bad_n}")
    eng.synchronize()
    assert (out.result("refusals") == FILL).all() and (big.cpu().numpy() == SENT).all()
    # adjacent ranges are fine: the destination begins where the source ends
    half = dev(eng, np.concatenate([src.cpu().numpy().ravel(), np.full(nbytes, FILL, np.uint8)]))
    assert P(half.data_ptr(), n, h, w, c, pm, h, w, half.data_ptr() + nbytes) == 0
    same(half.cpu().numpy()[nbytes:].reshape(n, h, w, c), src.cpu().numpy(), "adjacent ranges, identity")
    # the Python layer raises the library's error
    from icepy4d_amd._lib import IcematchError
    with pytest.raises(IcematchError) as ei:
        eng.ctx.call("im_undistort_image", ps, n, h, w, c, pr, ps, s)
    assert ei.value.rc == REFUSED and "overlap" in str(ei.value)
