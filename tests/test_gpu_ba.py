"""The bundle-adjustment kernels (csrc/ba.hip: im_ba_accumulate, im_ba_solve, im_ba_step_points, im_ba_decide, im_ba_residuals) on the
device on the shared cases (tests/ba_cases.py: point counts around the wave, the LDS tile and the chunk, absent observations, non-finite
values, a point behind a camera, full and partial priors, every mask extreme, a world frame, a planted singular system, a run with accepted
and rejected steps, a cost tolerance and a lambda ceiling that end a run, a three-epoch table), the whole loop through the Python layer
with the statuses as the device returns them, `bundle_adjust_table` on a gathered match table of 0, 65 and BA_CHUNK + 1 matches (from
the table on the device and with the reconstruction given, against `bundle_adjust` on every record and the restatement), and the refusals.

Bounds. Every output of the five entry points and every record of `bundle_adjust` / `bundle_adjust_epochs` (`history`): equality of bits
with the restatement (tests/ba_oracle.py), a NaN equal to a NaN whatever its payload. Derived, not measured: every sum runs in an order
fixed by the point index alone (a chunk's points ascending, then the chunks ascending: csrc/ba_point.h) over the same IEEE float64
operations with contraction off, and float64 division and sqrt are correctly rounded on the device. The host build of the same text agrees
with the restatement on the same cases (tests/test_ba_cpu.py); what only this file can show is the LDS exchange, the launch shapes, the
double buffering and a lost `#pragma clang fp contract(off)`.

Every output of a C ABI call lies between two guard bands of sentinel bytes in one allocation and is itself pre-filled; the bands must
come back untouched. Resuming: `bundle_adjust(state=...)` continues a run from a returned state, so a run split into k iterations and the
rest is compared with one run."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ba_cases as BC  # noqa: E402
import ba_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

BAND, SENT, FILL = 4096, 0xA5, 0x5A
REFUSED = -82


@pytest.fixture(scope="module")
def eng():
    from icepy4d_amd.engine import Engine
    e = Engine(0)
    yield e
    e.synchronize()


def p(t):
    from icepy4d_amd._lib import ptr
    return ptr(t)


def dev(eng, a):
    """A copy on the device (the shared inputs are read-only); an empty array becomes one zero row, so that its pointer is not null."""
    import torch
    a = np.array(a, order="C")
    if a.shape[0] == 0:
        a = np.zeros((1,) + a.shape[1:], a.dtype)
    return torch.from_numpy(a).to(eng.device)


def same(a, b):
    """Equality of bits, a NaN equal to a NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


class Framed:
    """An output of `shape` float64 between two bands of sentinel bytes, in one device allocation, pre-filled (or holding `init`)."""

    def __init__(self, eng, shape, init=None):
        import torch
        self.shape = tuple(shape)
        self.n = int(np.prod(self.shape, dtype=np.int64)) * 8
        host = np.full(2 * BAND + self.n, SENT, np.uint8)
        host[BAND:BAND + self.n] = FILL if init is None else np.ascontiguousarray(init, np.float64).reshape(-1).view(np.uint8)
        self.buf = torch.from_numpy(host).to(eng.device)
        self.ptr = self.buf.data_ptr() + BAND

    def result(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all(), (what, "a byte outside the output was written")
        return host[BAND:BAND + self.n].view(np.float64).reshape(self.shape)

    def untouched(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == SENT).all() and (host[BAND + self.n:] == SENT).all() and (host[BAND:BAND + self.n] == FILL).all(), what


class Table:
    """Epochs one behind the other on the device, every array the kernels write framed. parity: the buffers the epochs' state starts in."""

    def __init__(self, eng, names, parity=0, lam=None):
        t = BC.table(names)
        self.names, self.off, self.E, self.M = names, t["off"], len(names), int(t["off"][-1])
        self.max_points = int(np.diff(t["off"]).max())
        self.slots = self.M // O.BA_CHUNK + self.E + 1
        m = max(self.M, 1)
        pts2, cams2 = np.full((2, m, 3), -7.0), np.full((2, self.E, 48), -7.0)
        pts2[parity, :self.M], cams2[parity] = t["X"], t["cams"]
        self.parity = parity
        self.pts2, self.cams2 = Framed(eng, pts2.shape, pts2), Framed(eng, cams2.shape, cams2)
        self.doff, self.obs, self.sig, self.prior = dev(eng, t["off"]), dev(eng, t["obs"]), dev(eng, t["sig"]), dev(eng, t["prior"])
        self.cprior = dev(eng, t["cprior"])
        st = np.zeros((self.E, O.STATE))
        for e, n in enumerate(names):
            st[e] = O.initial_state(BC.by_name(n)["lam"] if lam is None else lam)
            st[e, O.ST_PARITY] = parity
        self.state = Framed(eng, st.shape, st)
        self.parts, self.cparts = Framed(eng, (self.slots, O.TERMS)), Framed(eng, (self.slots,))
        self.sol, self.res = Framed(eng, (self.E, O.SOL)), Framed(eng, (m, 2, 3))
        self.mask, self.opts = int(BC.by_name(names[0])["mask"]), np.ascontiguousarray(BC.by_name(names[0])["opts"])

    def slot(self, e):
        return int(self.off[e]) // O.BA_CHUNK + e

    def iteration(self, eng, history, own_scratch=True):
        s, c = eng.stream_ptr(), eng.ctx.call
        parts, cparts = (self.parts.ptr, self.cparts.ptr) if own_scratch else (None, None)
        c("im_ba_accumulate", p(self.doff), self.E, self.M, self.max_points, self.pts2.ptr, p(self.obs), p(self.sig), p(self.prior), self.cams2.ptr,
          self.state.ptr, parts, s)
        c("im_ba_solve", p(self.doff), self.E, self.M, parts, self.cams2.ptr, p(self.cprior), self.state.ptr, self.mask, self.sol.ptr, s)
        c("im_ba_step_points", p(self.doff), self.E, self.M, self.max_points, self.pts2.ptr, p(self.obs), p(self.sig), p(self.prior), self.cams2.ptr,
          self.state.ptr, self.sol.ptr, cparts, s)
        c("im_ba_decide", p(self.doff), self.E, self.M, cparts, self.cams2.ptr, p(self.cprior), self.state.ptr, self.sol.ptr, self.opts.ctypes.data,
          history.ptr, history.shape[0], s)

    def check_first_iteration(self, eng, what, own_scratch=True):
        """One iteration of every epoch against the restatement: partials, sums, draft, candidate cameras and points, cost partials, record,
        state; the bytes no epoch owns stay as they were."""
        history = Framed(eng, (int(self.opts[3]), self.E, O.RECORD))
        self.iteration(eng, history, own_scratch)
        par = self.parity
        pts2, cams2 = self.pts2.result(what), self.cams2.result(what)
        st, sol, hist = self.state.result(what), self.sol.result(what), history.result(what)
        if own_scratch:
            parts, cparts = self.parts.result(what), self.cparts.result(what)
        for e, name in enumerate(self.names):
            w, a, b, ch, sl = BC.first_iteration(name), int(self.off[e]), int(self.off[e + 1]), O.n_chunks(len(BC.by_name(name)["X"])), self.slot(e)
            if own_scratch:
                assert same(parts[sl:sl + ch], w["parts"]), (what, name, "partials")
                assert same(cparts[sl:sl + ch], w["cparts"]), (what, name, "cost partials")
            assert same(sol[e, :O.TERMS], w["sums"]) and not np.signbit(sol[e, :O.TERMS][sol[e, :O.TERMS] == 0.0]).any(), (what, name, "sums")
            assert same(sol[e, O.SOL_REC:], w["draft"]), (what, name, "draft")
            assert same(cams2[1 - par, e], w["cand"]) and same(cams2[par, e], BC.by_name(name)["cams"]), (what, name, "cameras")
            assert same(pts2[1 - par, a:b], w["cand_pts"]) and same(pts2[par, a:b], BC.by_name(name)["X"]), (what, name, "points")
            assert same(hist[0, e], w["rec"]) and (hist[1:, e].view(np.uint8) == FILL).all(), (what, name, "record")
            want_st = np.array(w["state"])
            want_st[O.ST_PARITY] = par if not w["accepted"] else 1 - par
            assert same(st[e], want_st), (what, name, "state", st[e], want_st)
        if own_scratch:
            owned = np.zeros(self.slots, bool)
            for e, name in enumerate(self.names):
                owned[self.slot(e):self.slot(e) + O.n_chunks(len(BC.by_name(name)["X"]))] = True
            assert (parts[~owned].view(np.uint8) == FILL).all() and (cparts[~owned].view(np.uint8) == FILL).all(), (what, "a slot no chunk owns")


# ---- the C entry points ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BC.names())
def test_one_iteration_equals_the_restatement(eng, name):
    Table(eng, (name,)).check_first_iteration(eng, name)


@pytest.mark.parametrize("parity", [0, 1])
def test_the_table_equals_its_epochs_in_any_order_and_either_buffer(eng, parity):
    Table(eng, BC.TABLE, parity).check_first_iteration(eng, f"table parity {parity}")
    Table(eng, BC.TABLE[::-1] + ("absent", "n0", "world"), parity).check_first_iteration(eng, f"permuted table parity {parity}")


def test_the_contexts_scratch_gives_the_same(eng):
    Table(eng, BC.TABLE + ("n513",)).check_first_iteration(eng, "context scratch", own_scratch=False)


@pytest.mark.parametrize("name", BC.names())
def test_residuals_equal_the_restatement(eng, name):
    t = Table(eng, ("n65", name))
    eng.ctx.call("im_ba_residuals", p(t.doff), t.E, t.M, t.max_points, t.pts2.ptr, p(t.obs), t.cams2.ptr, t.state.ptr, t.res.ptr, eng.stream_ptr())
    res = t.res.result(name)
    for e, nm in enumerate(t.names):
        c = BC.by_name(nm)
        assert same(res[int(t.off[e]):int(t.off[e + 1])], O.residuals(c["cams"], c["X"], c["obs"])), (name, nm)
    if name == "absent":
        assert np.isnan(res[65 + 5, 0]).all() and np.isfinite(res[65 + 5, 1]).all()
    t.pts2.result(name), t.cams2.result(name)


def test_a_finished_epoch_is_left_alone(eng):
    t = Table(eng, ("n65", "n257"))
    st = t.state.result("state").copy()
    st[1, O.ST_DONE], st[1, O.ST_STATUS] = 1.0, O.OK
    t.state = Framed(eng, st.shape, st)
    history = Framed(eng, (int(t.opts[3]), 2, O.RECORD))
    t.iteration(eng, history)
    parts, sol, hist, pts2 = t.parts.result("parts"), t.sol.result("sol"), history.result("history"), t.pts2.result("pts")
    assert same(hist[0, 0], BC.first_iteration("n65")["rec"])
    assert (parts[t.slot(1):].view(np.uint8) == FILL).all() and (sol[1].view(np.uint8) == FILL).all() and (hist[0, 1].view(np.uint8) == FILL).all()
    assert (pts2[1, 65:] == -7.0).all() and same(t.state.result("state")[1], st[1])


# ---- the whole loop through the Python layer ------------------------------------------------------------------------------------------------------
def _problem(name):
    c = BC.by_name(name)
    return {k: np.array(c[k]) for k in ("cams", "X", "obs", "sig", "prior", "cprior")}


def _check_run(out, name, max_iter=30):
    cams, X, st, hist = BC.whole_run(name, max_iter)
    c = BC.by_name(name)
    assert same(out[3], hist), (name, "history")
    assert same(out[0], cams) and same(out[1], X), (name, "final state")
    want = np.array(st)
    want[O.ST_PARITY] = out[2][O.ST_PARITY]                                # which buffer holds the result is the device's business
    assert same(out[2], want), (name, out[2], want)
    assert same(out[4], O.residuals(cams, X, c["obs"])), (name, "residuals")


DEVICE_STATUS = {"n0": O.EMPTY, "singular": O.DEGENERATE, "accept_reject": O.OK, "noisy": O.OK, "ctol": O.OK, "stalled": O.STALLED, "mask_fixed": O.OK}


@pytest.mark.parametrize("name", ["n0", "n65", "n257", "absent", "partial_priors", "mask_fixed", "world", "singular", "accept_reject", "noisy", "ctol", "stalled"])
def test_whole_loop_equals_the_restatement(eng, name):
    """The device's own history and state: equal to the restatement's, and the statuses and both paths of the decision occur ON THE DEVICE."""
    from icepy4d_amd import sfm
    c = BC.by_name(name)
    out = sfm.ba_run_device([_problem(name)], c["mask"], c["lam"], c["opts"], engine=eng)[0]
    _check_run(out, name)
    if name in DEVICE_STATUS:
        assert out[2][O.ST_STATUS] == DEVICE_STATUS[name] and out[2][O.ST_DONE] == 1.0, (name, out[2])
    acc = out[3][:, O.REC_ACCEPTED]
    if name == "accept_reject":
        assert (acc[:8] == 1.0).any() and (acc[:8] == 0.0).any()
    if name == "stalled":
        assert acc[-1] == 0.0 and out[3][-1, O.REC_LAMBDA] * 10.0 > c["opts"][1] and out[3][-1, O.REC_STATUS] == O.STALLED
    if name == "ctol":
        assert acc[-1] == 1.0 and 0.0 < out[3][-1, O.REC_COST1] <= c["opts"][4] and out[3][-1, O.REC_COST0] - out[3][-1, O.REC_COST1] > c["opts"][2] * out[3][-1, O.REC_COST0]
    if name in ("n0", "singular"):
        assert len(out[3]) == 1 and same(out[0], c["cams"]) and same(out[1], c["X"])           # the state stays


def test_the_table_run_equals_the_per_epoch_runs(eng):
    from icepy4d_amd import sfm
    c = BC.by_name(BC.TABLE[0])
    outs = sfm.ba_run_device([_problem(n) for n in BC.TABLE], c["mask"], c["lam"], c["opts"], engine=eng)
    for name, out in zip(BC.TABLE, outs):
        _check_run(out, name)
        alone = sfm.ba_run_device([_problem(name)], c["mask"], c["lam"], c["opts"], engine=eng)[0]
        assert all(same(a, b) for a, b in zip(out[:2] + out[3:], alone[:2] + alone[3:])), name


def test_max_iter_and_a_resumed_run(eng):
    from icepy4d_amd import sfm
    c = BC.by_name("noisy")
    opts3 = np.array(c["opts"])
    opts3[3] = 3
    first = sfm.ba_run_device([_problem("noisy")], c["mask"], c["lam"], opts3, engine=eng)[0]
    _check_run(first, "noisy", 3)
    assert first[2][O.ST_STATUS] == O.MAX_ITER and len(first[3]) == 3
    again = dict(_problem("noisy"), cams=first[0], X=first[1])
    rest = sfm.ba_run_device([again], c["mask"], c["lam"], c["opts"], states=[first[2]], engine=eng)[0]
    whole = BC.whole_run("noisy")
    first[3][-1, O.REC_STATUS] = O.RUNNING                                 # the one run did not stop there; everything else is the same
    assert same(np.concatenate([first[3], rest[3]]), whole[3]) and same(rest[0], whole[0]) and same(rest[1], whole[1])
    assert rest[2][O.ST_STATUS] == O.OK


def _cameras(c):
    from icepy4d_amd.core.camera import Camera
    cams = []
    for k in range(2):
        s = c["cams"][24 * k:24 * k + 24]
        K = np.array([[s[12], 0, s[14]], [0, s[13], s[15]], [0, 0, 1.0]])
        R, C = s[:9].reshape(3, 3), s[9:12].reshape(3, 1)
        cams.append(Camera(6000, 4000, K=K, dist=np.array(s[16:24]), R=R, t=-(R @ C)))
    return cams


def match_table(c, counts, K, seed=3):
    """A gathered match table with the keypoint payload: record e holds counts[e] matches among the tie points of case c, at scattered
    keypoint-0 slots and permuted keypoint-1 slots; the keypoints are the case's observations as float32."""
    from icepy4d_amd.sequence import HEADER, record_words
    rng = np.random.default_rng(seed)
    table = np.full((len(counts), record_words(K, True)), -1, np.int32)
    n_tie = len(c["X"]) - BC.N_CONTROL
    for e, n in enumerate(counts):
        sel = np.sort(rng.choice(n_tie, n, replace=False))
        slots0, perm1 = np.sort(rng.choice(K, n, replace=False)), rng.permutation(K)[:n]
        k0, k1 = np.zeros((K, 2), np.float32), np.zeros((K, 2), np.float32)
        k0[slots0], k1[perm1] = c["obs"][sel, :2], c["obs"][sel, 2:]
        m0 = np.full(K, -1, np.int32)
        m0[slots0] = perm1
        table[e, :5] = [e, K, K, n, 0]
        table[e, HEADER:HEADER + K] = m0
        table[e, HEADER + K:HEADER + 2 * K] = 0
        table[e, HEADER + 2 * K:] = np.concatenate([k0, k1]).reshape(-1).view(np.int32)
    return table


def test_bundle_adjust_table_on_the_three_epoch_table(eng):
    """0, 65 and BA_CHUNK + 1 matches: `bundle_adjust_table` from the table on the device (its own triangulation, keypoints gathered on
    the device, targets laid behind every epoch) and with the reconstruction given, against `bundle_adjust` on every record alone and
    against the restatement on the record's host-decoded keypoints and `triangulate_table`'s points: histories, points, residuals, bits."""
    import torch
    from icepy4d_amd import sfm
    c = BC.scene(O.BA_CHUNK + 1 + BC.N_CONTROL, seed=31, noise=0.5)
    cams, K, counts = _cameras(c), 320, (0, 65, O.BA_CHUNK + 1)
    table = match_table(c, counts, K)
    n = len(c["X"]) - BC.N_CONTROL
    kw = dict(targets=([c["obs"][n:, :2], c["obs"][n:, 2:]], c["prior"][n:, :3]), camera_centers_world=(c["cprior"][0:3], c["cprior"][6:9]),
              image_sigma=0.5)
    got = sfm.bundle_adjust_table(torch.from_numpy(table).to(eng.device), K, cams, engine=eng, **kw)
    rec = sfm.triangulate_table(table, K, cams, engine=eng)
    given = sfm.bundle_adjust_table(table, K, cams, reconstruction=rec, engine=eng, **kw)
    uv = sfm.table_image_points(table, K)
    assert [len(x) for x in rec.points3d] == list(counts) == [len(p[0]) for p in uv] and all(np.isfinite(x).all() for x in rec.points3d)
    for e in range(3):
        pr = sfm.ba_problem(cams, uv[e], rec.points3d[e], kw["targets"], kw["camera_centers_world"], 0.5)
        want = O.run(pr["cams"], pr["X"], pr["obs"], pr["sig"], pr["prior"], pr["cprior"], O.MASK_DEFAULT, O.options(ftol=1e-9), O.initial_state(1e-3))
        alone = sfm.bundle_adjust(cams, uv[e], rec.points3d[e], engine=eng, **kw)
        for r in (got[e], given[e], alone):
            assert same(r.history, want[3]) and same(r.points3d, want[1]) and same(r.residuals, O.residuals(want[0], want[1], pr["obs"])), e
            assert r.status == O.STATUS_NAMES[int(want[2][O.ST_STATUS])] == "OK" and r.points3d.shape == (counts[e] + BC.N_CONTROL, 3)
            assert all(same(sfm._ba_camera_state(r.cameras[k])[12:], want[0][24 * k + 12:24 * k + 24]) for k in range(2))
    assert sfm.bundle_adjust_table(table[:0], K, cams, engine=eng, **kw) == []
    with pytest.raises(ValueError, match="does not belong"):
        sfm.bundle_adjust_table(table[:2], K, cams, reconstruction=rec, engine=eng, **kw)
    broken = table.copy()
    broken[1, 3] = 70                                                      # the header promises five matches more than matches0 holds
    short = sfm.bundle_adjust_table(broken, K, cams, engine=eng, **kw)[1]
    assert short.points3d.shape == (70 + BC.N_CONTROL, 3) and np.isnan(short.points3d[65:70]).all() and np.isnan(short.residuals[65:70]).all()
    assert same(short.history, got[1].history) and same(short.points3d[:65], got[1].points3d[:65])     # unusable rows change nothing


def test_bundle_adjust_returns_new_cameras(eng):
    from icepy4d_amd import sfm
    c = BC.by_name("noisy")
    cams = _cameras(c)
    before = [(np.array(cam.K), np.array(cam.extrinsics), np.array(cam.dist)) for cam in cams]
    n = len(c["X"]) - BC.N_CONTROL
    r = sfm.bundle_adjust(cams, [c["obs"][:n, :2], c["obs"][:n, 2:]], c["X"][:n], targets=([c["obs"][n:, :2], c["obs"][n:, 2:]], c["prior"][n:, :3]),
                          camera_centers_world=(c["cprior"][0:3], c["cprior"][6:9]), image_sigma=0.5, ftol=1e-12, engine=eng)
    for cam, (K, ext, dist) in zip(cams, before):
        assert np.array_equal(cam.K, K) and np.array_equal(cam.extrinsics, ext) and np.array_equal(cam.dist, dist)
    # the same call on the restatement (tests/test_ba_cpu.py runs it without a device): the same history, bit for bit
    pr = sfm.ba_problem(cams, [c["obs"][:n, :2], c["obs"][:n, 2:]], c["X"][:n], ([c["obs"][n:, :2], c["obs"][n:, 2:]], c["prior"][n:, :3]),
                        (c["cprior"][0:3], c["cprior"][6:9]), 0.5)
    want = O.run(pr["cams"], pr["X"], pr["obs"], pr["sig"], pr["prior"], pr["cprior"], O.MASK_DEFAULT, O.options(ftol=1e-12), O.initial_state(1e-3))
    assert r.status == "OK" and same(r.history, want[3]) and same(r.points3d, want[1]) and same(r.residuals, O.residuals(want[0], want[1], pr["obs"]))
    assert 0.7 < r.sigma0 < 1.3                                            # unit weight: the noise of 0.5 px is the sigma
    for k in range(2):
        assert same(sfm._ba_camera_state(r.cameras[k])[12:], want[0][24 * k + 12:24 * k + 24])
        assert np.abs(sfm._ba_camera_state(r.cameras[k])[:12] - want[0][24 * k:24 * k + 12]).max() <= 1e-9       # extrinsics pass through R C by BLAS


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_the_outputs_untouched(eng):
    from icepy4d_amd._lib import IcematchError
    t = Table(eng, ("n65",))
    s, history = eng.stream_ptr(), Framed(eng, (2, 1, O.RECORD))
    acc = [p(t.doff), 1, t.M, t.max_points, t.pts2.ptr, p(t.obs), p(t.sig), p(t.prior), t.cams2.ptr, t.state.ptr, t.parts.ptr, s]
    sol = [p(t.doff), 1, t.M, t.parts.ptr, t.cams2.ptr, p(t.cprior), t.state.ptr, t.mask, t.sol.ptr, s]
    dec = [p(t.doff), 1, t.M, t.cparts.ptr, t.cams2.ptr, p(t.cprior), t.state.ptr, t.sol.ptr, t.opts.ctypes.data, history.ptr, 2, s]
    res = [p(t.doff), 1, t.M, t.max_points, t.pts2.ptr, p(t.obs), t.cams2.ptr, t.state.ptr, t.res.ptr, s]

    def refused(name, args, **change):
        args = list(args)
        for k, v in change.items():
            args[int(k[1:])] = v
        with pytest.raises(IcematchError) as e:
            eng.ctx.call(name, *args)
        assert e.value.rc == REFUSED, (name, change, e.value)

    for k in (0, 4, 5, 6, 7, 8, 9):
        refused("im_ba_accumulate", acc, **{f"a{k}": None})
    refused("im_ba_accumulate", acc, a1=0)
    refused("im_ba_accumulate", acc, a1=65536)
    refused("im_ba_accumulate", acc, a2=-1)
    refused("im_ba_accumulate", acc, a2=(1 << 26) + 1)
    refused("im_ba_accumulate", acc, a3=t.M + 1)
    refused("im_ba_solve", sol, a7=1 << 28)
    refused("im_ba_solve", sol, a8=None)
    refused("im_ba_residuals", res, a8=None)
    for bad in ([0.0, 1e8, 1e-12, 30, 0], [1e-3, 1e-6, 1e-12, 30, 0], [1e-12, 1e8, -1.0, 30, 0], [1e-12, 1e8, 1e-12, 0, 0], [1e-12, 1e8, 1e-12, 3, 0],
                [1e-12, 1e8, 1e-12, 2, -1.0], [np.nan, 1e8, 1e-12, 2, 0]):
        refused("im_ba_decide", dec, a8=np.array(bad, np.float64).ctypes.data)
    big = Table(eng, ("n513", "n513", "n513", "n513"))                     # more than the context's scratch holds after the tables above
    with pytest.raises(IcematchError) as e:
        eng.ctx.call("im_ba_step_points", p(big.doff), big.E, 1 << 24, 1, big.pts2.ptr, p(big.obs), p(big.sig), p(big.prior), big.cams2.ptr,
                     big.state.ptr, big.sol.ptr, None, s)
    assert e.value.rc == REFUSED
    for f in (t.parts, t.cparts, t.sol, t.res, history):
        f.untouched("a refused call")
    assert same(t.state.result("state")[0], O.initial_state(1e-3)) and eng.ctx.lib.im_ba_chunk() == O.BA_CHUNK
