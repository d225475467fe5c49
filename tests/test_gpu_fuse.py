"""Depth-map fusion on the device: the two entry points of csrc/dense_fuse.hip on every case of tests/fuse_cases.py against the restatement
(tests/fuse_oracle.py) bit for bit, every output between two bands of sentinel bytes and pre-filled (`d_claimed` with 0xFF), every launch
run twice over its own result; the rest on the device's own `claimed` and on an uploaded one, so that a link bug cannot hide behind it;
`fuse` and `build_dense_cloud(fuse=...)` against the restatement's chain, and `fuse=None` against today's output; the -83 refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_oracle as O  # noqa: E402
import fuse_cases as C  # noqa: E402
import fuse_oracle as FO  # noqa: E402

from icepy4d_amd.dense import fuse  # noqa: E402,F401  (the feature under test: without it nothing here can pass)
from test_gpu_sgm import BAND, Framed, bits, dev  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


def fill(framed, byte):
    framed.buf[BAND:BAND + framed.n] = byte
    return framed


# ---- the two entry points ---------------------------------------------------------------------------------------------------------------------------
def run_link(eng, c, /, outs=None, **change):
    held = {k: dev(eng, c[k]) for k in ("keep_a", "w_a", "score_a", "keep_b", "w_b", "score_b")}
    (ha, wa), (hb, wb) = c["keep_a"].shape, c["keep_b"].shape
    outs = outs or (Framed(eng, (ha, wa), np.int32), Framed(eng, (ha, wa), np.float64), Framed(eng, (ha, wa), np.float32), Framed(eng, (ha, wa), np.uint8),
                    fill(Framed(eng, (hb, wb), np.uint8), 0xFF))
    pose = np.ascontiguousarray(c["pose_ab"], np.float64)
    a = dict({k: v.data_ptr() for k, v in held.items()}, ha=ha, wa=wa, hb=hb, wb=wb, pose=pose.ctypes.data, tol=float(c["tol_b"]), link=outs[0].ptr,
             w_out=outs[1].ptr, score_out=outs[2].ptr, views=outs[3].ptr, claimed=outs[4].ptr)
    a.update(change)
    for k, v in list(a.items()):
        if isinstance(v, str):                                                    # "=w_a": the pointer of another argument
            a[k] = a[v[1:]]
    rc = eng.ctx.lib.im_dense_fuse_link(eng.ctx.h, a["keep_a"], a["w_a"], a["score_a"], a["ha"], a["wa"], a["keep_b"], a["w_b"], a["score_b"], a["hb"], a["wb"],
                                        a["pose"], a["tol"], a["link"], a["w_out"], a["score_out"], a["views"], a["claimed"], eng.stream_ptr())
    eng.synchronize()
    return rc, outs


def run_rest(eng, c, claimed, /, out=None, **change):
    """`claimed`: a device address (the link's own output) or a host array, which is uploaded."""
    held = {k: dev(eng, c[k]) for k in ("keep_a", "w_a", "keep_b", "w_b")}
    if isinstance(claimed, np.ndarray):
        held["claimed"] = dev(eng, claimed)
        claimed = held["claimed"].data_ptr()
    (ha, wa), (hb, wb) = c["keep_a"].shape, c["keep_b"].shape
    out = out or Framed(eng, (hb, wb), np.uint8)
    pose = np.ascontiguousarray(c["pose_ba"], np.float64)
    a = dict(keep_b=held["keep_b"].data_ptr(), w_b=held["w_b"].data_ptr(), hb=hb, wb=wb, keep_a=held["keep_a"].data_ptr(), w_a=held["w_a"].data_ptr(), ha=ha,
             wa=wa, pose=pose.ctypes.data, tol=float(c["tol_a"]), claimed=claimed, rest=out.ptr)
    a.update(change)
    for k, v in list(a.items()):
        if isinstance(v, str):
            a[k] = a[v[1:]]
    rc = eng.ctx.lib.im_dense_fuse_rest(eng.ctx.h, a["keep_b"], a["w_b"], a["hb"], a["wb"], a["keep_a"], a["w_a"], a["ha"], a["wa"], a["pose"], a["tol"],
                                        a["claimed"], a["rest"], eng.stream_ptr())
    eng.synchronize()
    return rc, out


@pytest.mark.parametrize("name", list(C.cases()))
def test_both_entry_points_equal_the_restatement_and_repeat(eng, name):
    c, want = C.cases()[name], C.expected(name)
    rc, outs = run_link(eng, c)
    got = [o.result(name) for o in outs]
    assert rc == 0 and all(bits(g, w) for g, w in zip(got, want[:5])), (name, [int((g.view(np.uint8) != w.view(np.uint8)).sum()) for g, w in zip(got, want[:5])])
    rc, outs = run_link(eng, c, outs=outs)                                         # over its own result: the claims are cleared, then stored again
    again = [o.result(name) for o in outs]
    assert rc == 0 and all(bits(g, w) for g, w in zip(again, got)), name
    for claimed in (outs[4].ptr, want[4]):                                        # the device's own claims, then uploaded ones
        rc, out = run_rest(eng, c, claimed)
        rest = out.result(name)
        assert rc == 0 and bits(rest, want[5]), (name, int((rest != want[5]).sum()))
        rc, out = run_rest(eng, c, claimed, out=out)
        assert rc == 0 and bits(out.result(name), rest), name


def test_the_rest_follows_the_claims_it_is_given(eng):
    """With nothing claimed, every kept pixel of view b without a link of its own is left; with everything claimed, none is."""
    c = C.cases()["swept_rotated_NoFiltering_base0"]
    for claimed in (np.zeros_like(c["keep_b"]), np.ones_like(c["keep_b"])):
        rc, out = run_rest(eng, c, claimed)
        assert rc == 0 and bits(out.result("claims"), FO.rest(c["keep_b"], c["w_b"], c["keep_a"], c["w_a"], c["pose_ba"], c["tol_a"], claimed))


# ---- the Python layers ------------------------------------------------------------------------------------------------------------------------------
def restated_fusion(maps, a, depth_filter, tol, min_views):
    """The restatement's chain behind the sweep: consistency both ways, the fusion, the cloud of the base and of the rest."""
    b = 1 - a
    tau = O.filter_tau(depth_filter)
    keep, pose, cam = {}, {}, {}
    for v, o in ((a, b), (b, a)):
        R, t = O.relative_pose(maps[v]["R"], maps[v]["t"], maps[o]["R"], maps[o]["t"])
        pose[v] = np.concatenate([O.W.inv3(maps[v]["K"]).reshape(9), R.reshape(9), t, maps[o]["K"].reshape(9)])
        keep[v] = O.consistency(maps[v]["out"][0], maps[v]["out"][1], maps[o]["out"][0], maps[o]["out"][1], pose[v],
                                0.0 if tau is None else tau * abs(maps[o]["w_step"]), tau is not None)
        cam[v] = np.concatenate([O.W.inv3(maps[v]["K"]).reshape(9), maps[v]["R"].reshape(9), maps[v]["t"]])
    tol_b, tol_a = tol * abs(maps[b]["w_step"]), tol * abs(maps[a]["w_step"])
    fused = FO.fuse(keep[a], maps[a]["out"][1], maps[a]["out"][2], keep[b], maps[b]["out"][1], maps[b]["out"][2], pose[a], tol_b)
    rest = FO.rest(keep[b], maps[b]["out"][1], keep[a], maps[a]["out"][1], pose[b], tol_a, fused[4])
    cloud = FO.fused_cloud(keep[a], maps[a]["out"][1:], maps[a]["image"], cam[a], keep[b], maps[b]["out"][1:], maps[b]["image"], cam[b], pose[a], pose[b],
                           tol_b, tol_a, min_views)
    return keep, fused, rest, cloud


@pytest.mark.parametrize("downscale", [1, 2])
@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
def test_python_layers_equal_the_restatements_chain(eng, downscale, rgb):
    from icepy4d_amd import dense as D
    import test_gpu_dense as TD
    images, cams, rng = TD.python_pair(rgb)
    want_maps = TD.restated_maps(images, cams, rng, downscale, 2, 0.6)
    opts = dict(depth_filter="MildFiltering", downscale=downscale, depth_range=rng, radius=2, min_score=0.6, engine=eng)
    maps = D.build_depth_maps(images, cams, depth_range=rng, downscale=downscale, radius=2, min_score=0.6, engine=eng)
    for base, tol, min_views in ((0, 1.0, 1), (1, 1.0, 1), (0, 1.0, 2), (1, 0.5, 2)):
        other = 1 - base
        keep, fused, rest, cloud = restated_fusion(want_maps, base, "MildFiltering", tol, min_views)
        assert (fused[3] == 2).sum() > 100 and (fused[3] == 1).sum() > 0 and rest.sum() > 0               # every kind of pixel occurs
        k = [D.consistency(maps[v], maps[1 - v], "MildFiltering", engine=eng) for v in (0, 1)]
        m, views, link, left = fuse(maps[base], k[base], maps[other], k[other], tol, engine=eng)
        got = (link.cpu().numpy(), m.w.cpu().numpy(), m.score.cpu().numpy(), views.cpu().numpy())
        assert all(bits(g, w) for g, w in zip(got, fused[:4])) and bits(left.cpu().numpy(), rest), (base, tol)
        assert bits(m.plane.cpu().numpy(), want_maps[base]["out"][0]) and bits(maps[base].w.cpu().numpy(), want_maps[base]["out"][1])     # the input is as it was
        pcd = D.build_dense_cloud(images, cams, views=(base, other), fuse=(tol, min_views), **opts)
        assert len(cloud[0]) > 100 and len(pcd) == len(cloud[0])
        assert bits(pcd.points, cloud[0]) and bits(pcd.colors, cloud[1].astype(np.float64) / 255.0) and bits(pcd.normals, cloud[2])
        assert bits(pcd.confidence, cloud[3]) and bits(pcd.views, cloud[4])
        # aligned with the points: the scalars of the base's part are the fused map's at the pixels the mask names, in row-major order
        mask = fused[3] >= min_views
        assert len(pcd.views) == len(pcd.confidence) == len(pcd) and np.array_equal(pcd.views[:mask.sum()], fused[3][mask])
        assert np.array_equal(pcd.confidence[:mask.sum()], fused[2][mask]) and (pcd.views[mask.sum():] == 1).all()
        assert (len(pcd) == mask.sum() + rest.sum()) if min_views == 1 else (len(pcd) == mask.sum() and (pcd.views == 2).all())
    plain = D.build_dense_cloud(images, cams, views=(0, 1), **opts)
    none = D.build_dense_cloud(images, cams, views=(0, 1), fuse=None, **opts)
    assert bits(plain.points, none.points) and bits(plain.colors, none.colors) and bits(plain.normals, none.normals) and bits(plain.confidence, none.confidence)
    assert plain.views is None and none.views is None and len(plain) > len(cloud[0])
    xyz = np.concatenate([TD.restated_cloud(want_maps, v, "MildFiltering")[0] for v in (0, 1)])
    assert bits(none.points, xyz)                                                 # today's cloud, bit for bit


def test_a_fused_cloud_is_written_with_its_scalars(eng, tmp_path):
    from icepy4d_amd import dense as D
    from icepy4d_amd.core.point_cloud import PointCloud
    import test_gpu_dense as TD
    images, cams, rng = TD.python_pair(True)
    out = D.dense_series([images], cams, out_dir=tmp_path, dates=["2022_05_01"], depth_range=rng, radius=2, min_score=0.6, engine=eng, views=(0, 1),
                         fuse=(1.0, 1), ply_scalars=("confidence", "views"))
    with open(tmp_path / "dense_2022_05_01.ply", "rb") as f:
        head = f.read().split(b"end_header\n")[0].decode("ascii").splitlines()
    assert head[-2:] == ["property float confidence", "property uchar views"] and set(np.unique(out[0].views)) == {1, 2}
    back = PointCloud(pcd_path=str(tmp_path / "dense_2022_05_01.ply"))
    assert len(back) == len(out[0]) > 100 and bits(back.points, out[0].points) and bits(back.normals, out[0].normals)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------
INPUTS = ("keep_a", "w_a", "score_a", "keep_b", "w_b", "score_b")
LINK_REFUSALS = ([{k: None} for k in INPUTS + ("pose", "link", "w_out", "score_out", "views", "claimed")]
                 + [dict(ha=0), dict(ha=16385), dict(wa=0), dict(wa=16385), dict(hb=0), dict(hb=16385), dict(wb=0), dict(wb=16385),
                    dict(tol=-1e-300), dict(tol=float("nan")), dict(tol=float("-inf"))]
                 + [{out: "=" + src} for out, src in (("w_out", "w_a"), ("w_out", "w_b"), ("score_out", "score_a"), ("score_out", "score_b"), ("views", "keep_a"),
                                                      ("claimed", "keep_b"), ("link", "w_a"), ("views", "keep_b"), ("claimed", "keep_a"))])
REST_REFUSALS = ([{k: None} for k in ("keep_b", "w_b", "keep_a", "w_a", "pose", "claimed", "rest")]
                 + [dict(ha=0), dict(wa=16385), dict(hb=16385), dict(wb=0), dict(tol=-1.0), dict(tol=float("nan"))]
                 + [{"rest": "=" + src} for src in ("keep_b", "w_b", "keep_a", "w_a", "claimed")])


def ids(changes):
    return [",".join(f"{k}={v}" for k, v in c.items()) for c in changes]


@pytest.mark.parametrize("change", LINK_REFUSALS, ids=ids(LINK_REFUSALS))
def test_link_refusals_launch_nothing(eng, change):
    c = C.cases()["shape_17x65"]
    rc, outs = run_link(eng, c, **change)
    assert rc == -83
    for o in outs[:4]:
        o.untouched(change)
    host = outs[4].buf.cpu().numpy()                                              # the claims were pre-filled with 0xFF: not even the clear ran
    assert (host[BAND:BAND + outs[4].n] == 0xFF).all() and (host[:BAND] == 0xA5).all() and (host[BAND + outs[4].n:] == 0xA5).all(), change


@pytest.mark.parametrize("change", REST_REFUSALS, ids=ids(REST_REFUSALS))
def test_rest_refusals_launch_nothing(eng, change):
    name = "shape_17x65"
    rc, out = run_rest(eng, C.cases()[name], C.expected(name)[4], **change)
    assert rc == -83
    out.untouched(change)
