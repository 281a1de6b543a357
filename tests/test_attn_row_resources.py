"""The row attention kernels (csrc/kernels/attention_row.hip) must fit their waves per workgroup
without spilling: the four backward instantiations use no scratch and no more VGPRs or LDS than
measured at commit 6dad863, the three forward instantiations no scratch and at most 128 / 128 / 223
VGPRs.  Compiled for gfx950 with the build's own flags plus the compiler's resource-usage remarks
(about 5 s); only the remarks are read."""
import os
import re
import subprocess

import pytest

from textsummarization_on_flink_amd import _build

# kernel<NK, NW>: (VGPRs, LDS bytes) at 6dad863
BWD = {
    ("attn_bwd_row_kernel", 1, 12): (140, 32816),
    ("attn_bwd_row_kernel", 2, 8): (252, 49184),
    ("attn_bwd_rowp_kernel", 1, 16): (122, 39488),
    ("attn_bwd_rowp_kernel", 2, 8): (198, 45600),
}
# attn_fwd_row_kernel<NK, NW, PROBE = 0>: VGPRs
FWD = {
    ("attn_fwd_row_kernel", 1, 12): 128,
    ("attn_fwd_row_kernel", 1, 16): 128,
    ("attn_fwd_row_kernel", 2, 8): 223,
}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(_build.HIPCC):
        pytest.skip("hipcc is not installed")
    src = os.path.join(_build.CSRC, "kernels", "attention_row.hip")
    obj = tmp_path_factory.mktemp("attn_row") / "ar.o"
    cmd = [_build.HIPCC, *_build.kernel_flags(), "-c", src, "-o", str(obj),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: +([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            # _Z<len><name>ILi<NK>ELi<NW>E[Li<PROBE>E]E...
            t = re.match(r"_Z\d+([a-z_]+)ILi(\d+)ELi(\d+)E(?:Li(\d+)E)?E", val)
            assert t, val
            cur = res.setdefault((t.group(1), int(t.group(2)), int(t.group(3)), int(t.group(4) or 0)), {})
        elif cur is not None:
            cur[key] = int(val) if val.isdigit() else val
    return res


def _no_spill(k):
    assert k["ScratchSize"] == 0
    assert k["VGPRs Spill"] == 0
    assert k["SGPRs Spill"] == 0


@pytest.mark.parametrize("kern", sorted(BWD), ids=lambda k: "%s-%d-%d" % k)
def test_attn_bwd_row_resources(remarks, kern):
    k = remarks[kern + (0,)]
    print(kern, k)
    _no_spill(k)
    vgprs, lds = BWD[kern]
    assert k["VGPRs"] <= vgprs
    assert k["LDS Size"] <= lds


@pytest.mark.parametrize("kern", sorted(FWD), ids=lambda k: "%s-%d-%d" % k)
def test_attn_fwd_row_resources(remarks, kern):
    k = remarks[kern + (0,)]
    print(kern, k)
    _no_spill(k)
    assert k["VGPRs"] <= FWD[kern]
