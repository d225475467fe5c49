"""The 64-row projection blocks that write K / V straight as the attention's bf16 planes (csrc/proj_planes.hip) against the path they replace:
`IM_PROJ_ROWS32=1` = the 32-row blocks of gemm.hip (fp32 q / k / v) followed by `kv_planes_kernel`. Same products in the same order per accumulator,
the same epilogue statements, the same cut: every byte must be equal, and nothing at or past an image's live row count may be written."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -777.25      # fp32 buffers
SENTINEL_BYTE = 0xA5    # plane buffers


@pytest.fixture(scope="module")
def ctx():
    from icepy4d_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def weights():
    """Seeded projection weights on the host: Wqkv [768][256] and [to_qk ; to_v] [512][256] with their biases."""
    g = torch.Generator().manual_seed(10)
    return {0: (torch.randn(768, 256, generator=g) / 16, torch.randn(768, generator=g) * 0.1),
            1: (torch.randn(512, 256, generator=g) / 16, torch.randn(512, generator=g) * 0.1)}


def run(ctx, monkeypatch, rows32, cross, w, b, x, cs, sn, n, active, n_max, attention=False):
    """One call of the stage entry: (q, k, v, planes, att) with everything poisoned before the launch."""
    from icepy4d_amd._lib import ptr, stream_ptr
    if rows32:
        monkeypatch.setenv("IM_PROJ_ROWS32", "1")
    else:
        monkeypatch.delenv("IM_PROJ_ROWS32", raising=False)
    ni = x.shape[0]
    q, k, v = (torch.full((ni, 4, n_max, 64), SENTINEL, device="cuda") for _ in range(3))
    planes = torch.full((2, ni, 4, n_max, 3, 128), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    att = torch.full((ni, n_max, 256), SENTINEL, device="cuda") if attention else None
    ctx.call("im_block_proj_attn", cross, ptr(x), ptr(w), ptr(b), ptr(cs), ptr(sn), 0.35355339059327373, ptr(n), ptr(active), ni // 2, n_max,
             ptr(q), ptr(k), ptr(v), ptr(planes), ptr(att), 1.0 if cross else 0.125, stream_ptr())
    torch.cuda.synchronize()
    return q, k, v, planes, att


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("n_max", [1, 31, 32, 33, 63, 64, 65, 130])
def test_planes_from_the_projection_equal_the_plane_pass(ctx, weights, monkeypatch, n_max, cross):
    """Three pairs per launch: (full, n_max - 1), (0 live rows, full) and one pair with active = 0. q, the K planes and the V planes of the new
    path equal those of the 32-row projection + plane pass bit for bit; rows at or past the live count and the inactive pair keep the poison;
    the new path does not write fp32 k / v at all (the round trip this kernel removes). cross 0: q | k | v with rotary; cross 1: alpha * qk | v."""
    w, b = weights[cross]
    g = torch.Generator().manual_seed(100 * n_max + cross)
    x = torch.randn(6, n_max, 256, generator=g).cuda()
    ang = torch.rand(6, n_max, 32, generator=g) * 6.28
    cs, sn = (ang.cos().cuda(), ang.sin().cuda()) if not cross else (None, None)
    live = [n_max, n_max - 1, 0, n_max, n_max, n_max]
    n = torch.tensor(live, dtype=torch.int32).cuda()
    active = torch.tensor([1, 0, 1, 0, 0, 0], dtype=torch.int32).cuda()        # [pair][2]: the flag is the first int of a pair
    q0, k0, v0, p0, _ = run(ctx, monkeypatch, True, cross, w, b, x, cs, sn, n, active, n_max)
    q1, k1, v1, p1, _ = run(ctx, monkeypatch, False, cross, w, b, x, cs, sn, n, active, n_max)
    assert torch.equal(q0.view(torch.int32), q1.view(torch.int32))
    assert torch.equal(p0, p1)
    for z, m in enumerate(live):
        m = m if z < 4 else 0           # the inactive pair
        for q, p in ((q0, p0), (q1, p1)):
            assert (q[z, :, m:] == SENTINEL).all() and (p[:, z, :, m:] == SENTINEL_BYTE).all(), z
        if m:                           # the live rows were written: the planes are the cut of the values the old path stored as fp32
            src_k = q0 if cross else k0
            tri = p1[:, z, :, :m].contiguous().view(torch.int16).view(2, 4, m, 3, 64).to(torch.int32) << 16
            val = tri.view(torch.float32).double().sum(3)
            assert torch.equal(val[0], src_k[z, :, :m].double()) and torch.equal(val[1], v0[z, :, :m].double()), z
    assert (v1 == SENTINEL).all() and (k1 == SENTINEL).all()
    assert not (v0[0] == SENTINEL).any()


@pytest.mark.parametrize("cross", [0, 1])
def test_attention_of_a_block_is_bit_identical(ctx, weights, monkeypatch, cross):
    """One LightGlue block head, self and cross, 2 x 130 keypoints (one image a row short): projection, planes and attention through both paths."""
    w, b = weights[cross]
    n_max = 130
    g = torch.Generator().manual_seed(7 + cross)
    x = torch.randn(2, n_max, 256, generator=g).cuda()
    ang = torch.rand(2, n_max, 32, generator=g) * 6.28
    cs, sn = (ang.cos().cuda(), ang.sin().cuda()) if not cross else (None, None)
    n = torch.tensor([130, 129], dtype=torch.int32).cuda()
    outs = [run(ctx, monkeypatch, rows32, cross, w, b, x, cs, sn, n, None, n_max, attention=True) for rows32 in (True, False)]
    att0, att1 = outs[0][4], outs[1][4]
    assert torch.equal(att0.view(torch.int32), att1.view(torch.int32))
    assert (att1[1, 129:] == SENTINEL).all() and torch.isfinite(att1[0]).all() and torch.isfinite(att1[1, :129]).all()
    assert float(att1[0].abs().max()) > 1e-3
