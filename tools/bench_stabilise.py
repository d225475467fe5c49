"""Times the image stabilisation kernels of csrc/warp.hip on the device (device events, one warm-up, median of the repeats): the
workload of the reference's driver for one camera, `--frames` frames of 4008 x 6012 x 3 bytes, each undistorted with the first
calibration of the fixture (the reference's `assets/calib`, full size) and warped onto a reference camera by a rotation of up to half a
degree, as `stabilise_sequence` launches them: one `im_undistort_image` and one `im_warp_perspective` for all frames.

Reported per launch: milliseconds, milliseconds per frame, and the time a copy of the same bytes would take at the 6.3 TB/s copy rate
DESIGN uses, counting 6 bytes per pixel and pass (3 read, 3 written: what the kernel must move once; the four taps of neighbouring pixels
overlap and are expected from cache). Before timing, the top rows of frame 0 of both outputs are compared with the numpy restatement
(tests/warp_oracle.py) byte for byte: the production size reaches coordinates the small shapes of the test suite do not. The time of that
restatement on the host is reported next to the kernels', per frame by the pixel count: it is a PORT of the arithmetic to whole arrays,
not OpenCV and not the reference's run time.

    python tools/bench_stabilise.py [--frames 40] [--repeats 7] [--no-oracle] [--out profiles/r11_stabilise_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
COPY_RATE = 6.3e12
H, W_, C = 4008, 6012, 3


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def timed(torch, fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(m, 4) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--oracle-rows", type=int, default=96)
    ap.add_argument("--no-oracle", action="store_true", help="time only (timing ablations of the kernels do not compute the result)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_stabilise_bench.json"))
    a = ap.parse_args()
    assert a.repeats >= 5 and a.frames >= 1 and 1 <= a.oracle_rows <= H
    import torch
    import warp_oracle as W
    from icepy4d_amd.core import Camera
    from icepy4d_amd.engine import Engine
    from icepy4d_amd.utils import homography as hom
    if not torch.cuda.is_available():
        sys.exit("bench_stabilise.py needs a HIP device: there is nothing to time without one")
    eng = Engine(0)
    dev = eng.device
    n = a.frames
    with np.load(W.GOLDEN, allow_pickle=False) as g:
        K, dist = g["calib_cam1_K"], g["calib_cam1_dist"]
    rng = np.random.default_rng(11)
    R_ref = rot(0.31, -0.12, 0.05)
    cam_ref = Camera(W_, H, K, dist, R=R_ref, t=np.zeros(3))
    cams = []
    for _ in range(n):
        axis = rng.normal(size=3)
        R = rot(*(axis / np.linalg.norm(axis) * rng.uniform(0.1, 0.5) * np.deg2rad(1.0))) @ R_ref
        cams.append(Camera(W_, H, K, dist, R=R, t=np.zeros(3)))
    minv = np.stack([hom.inverse_homography(hom.homography(cam_ref, c)) for c in cams])
    h_cam = hom.undistort_params(cams[0])

    gen = torch.Generator(device=dev).manual_seed(11)
    src = torch.randint(0, 256, (n, H, W_, C), dtype=torch.uint8, device=dev, generator=gen)
    und = torch.empty_like(src)
    out = torch.empty_like(src)
    d_minv = torch.from_numpy(minv).to(dev)
    from icepy4d_amd._lib import ptr

    def undistort():
        eng.ctx.call("im_undistort_image", ptr(src), n, H, W_, C, h_cam.ctypes.data, ptr(und), eng.stream_ptr())

    def warp():
        eng.ctx.call("im_warp_perspective", ptr(und), n, H, W_, C, ptr(d_minv), H, W_, ptr(out), eng.stream_ptr())

    def both():
        undistort()
        warp()

    res = {"device": torch.cuda.get_device_name(0), "frames": n, "frame": [H, W_, C], "repeats": a.repeats, "copy_rate_bytes_per_s": COPY_RATE,
           "bytes_per_pixel_and_pass": 2 * C, "launches": {}}

    # ---- the production size against the restatement: the top rows of frame 0, both passes
    eq_und = eq_out = True
    if not a.no_oracle:
        both()
        torch.cuda.synchronize()
        rows = a.oracle_rows
        src0, und0 = src[0].cpu().numpy(), und[0].cpu().numpy()
        t0 = time.perf_counter()
        sx, sy = W.undistort_coords(h_cam[:9], h_cam[9:13], h_cam[13:], rows, W_)
        want_und = W.remap(src0, sx, sy)
        sx, sy = W.warp_coords(minv[0], rows, W_)
        want_out = W.remap(und0, sx, sy)
        dt = time.perf_counter() - t0
        eq_und = bool(np.array_equal(und0[:rows], want_und))
        eq_out = bool(np.array_equal(out[0, :rows].cpu().numpy(), want_out))
        res["oracle_port"] = dict(rows=rows, pixels=rows * W_, seconds_both_passes=round(dt, 3),
                                  seconds_per_frame_both_passes=round(dt * H / rows, 2), undistort_equal=eq_und, warp_equal=eq_out,
                                  nonzero_share_of_warped_rows=float((want_out != 0).mean()),
                                  note="numpy restatement on whole arrays (tests/warp_oracle.py), includes widening the source frame to int64; a port: "
                                       "not OpenCV, not the reference's run time")
        print(f"oracle port: {dt:.2f} s for {rows} rows of both passes ({dt * H / rows:.1f} s per frame); device equal: undistort {eq_und}, warp {eq_out}",
              flush=True)

    for name, fn, passes in (("undistort", undistort, 1), ("warp", warp, 1), ("undistort_then_warp", both, 2)):
        ms, all_ms = timed(torch, fn, a.repeats)
        nbytes = passes * n * H * W_ * 2 * C
        at_copy = nbytes / COPY_RATE * 1e3
        res["launches"][name] = dict(ms=round(ms, 3), ms_all=all_ms, ms_per_frame=round(ms / n, 4), bytes=int(nbytes),
                                     ms_at_copy_rate=round(at_copy, 3), fraction_of_copy_rate=round(at_copy / ms, 4),
                                     gpixels_per_s=round(passes * n * H * W_ / (ms * 1e-3) / 1e9, 2))
        print(f"{name:22s} {ms:9.3f} ms  {ms / n:8.4f} ms per frame  {at_copy / ms:6.3f} of the copy rate", flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    eng.close()
    if not (eq_und and eq_out):
        sys.exit("the device output differs from the restatement at the production size")


if __name__ == "__main__":
    main()
