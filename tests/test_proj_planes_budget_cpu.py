"""What csrc/proj_planes.hip is for, read off its gfx950 listing (no GPU needed): every kernel within 256 registers without spills or scratch,
and in the hot block of each twice as many bf16 MFMAs per weight-fragment load as in the hot block of gemm.hip's 32-row `proj_rows_kernel` -
each fragment in registers feeds two row groups, so the stream through the L1 -> register path per row is halved."""
import re

from toolchain import device_listing, kernel_body, kernel_resources

MFMA = "v_mfma_f32_32x32x16_bf16"


def mfma_per_load(listing, symbol):
    """(MFMAs, register loads of 16 bytes that are not LDS-DMA) in the basic block of `symbol` that holds the most MFMAs."""
    hot = max(re.split(r"\n\.LBB\d+_\d+:", kernel_body(listing, symbol)), key=lambda b: b.count(MFMA))
    loads = sum(1 for l in hot.split("\n") if l.strip().startswith("buffer_load_dwordx4") and not l.rstrip().endswith(" lds"))
    return hot.count(MFMA), loads


def test_proj_planes_kernels_keep_their_budget_and_halve_the_weight_stream(tmp_path):
    new = device_listing("proj_planes.hip", str(tmp_path))
    res = kernel_resources(new)
    assert len(res) >= 2 and all("proj_rows64_kernel" in k for k in res), sorted(res)
    for k, f in res.items():
        assert f["vgpr_count"] <= 256 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (k, dict(f))
    old = device_listing("gemm.hip", str(tmp_path))
    ratios_old = []
    for k in kernel_resources(old):
        if "proj_rows_kernel" in k:
            m, l = mfma_per_load(old, k)
            assert m > 0 and l > 0 and m % l == 0, (k, m, l)
            ratios_old.append(m // l)
    assert len(ratios_old) == 2 and len(set(ratios_old)) == 1, ratios_old
    for k in res:
        m, l = mfma_per_load(new, k)
        assert l > 0 and m == 2 * ratios_old[0] * l, (k, m, l)
