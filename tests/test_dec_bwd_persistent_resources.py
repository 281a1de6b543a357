"""dec_bwd_persistent_kernel (csrc/kernels/decoder_bwd_persistent.hip) is built with 16 waves per
workgroup, which the bit-equality with attn_bwd_rowp_kernel<1, 16> needs (the position groups and the
ds merge are dealt over the waves), so it must fit 128 VGPRs without spilling: 0 bytes of scratch, no
spilled VGPR.  Compiled for gfx950 with the build's own flags plus the compiler's resource-usage
remarks (about 5 s); only the remarks are read."""
import os
import re
import subprocess

import pytest

from textsummarization_on_flink_amd import _build


def test_dec_bwd_persistent_no_scratch(tmp_path):
    if not os.path.exists(_build.HIPCC):
        pytest.skip("hipcc is not installed")
    src = os.path.join(_build.CSRC, "kernels", "decoder_bwd_persistent.hip")
    cmd = [_build.HIPCC, *_build.kernel_flags(), "-c", src, "-o", str(tmp_path / "dbp.o"),
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
            cur = res.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    (kern,) = [v for n, v in res.items() if "dec_bwd_persistent_kernel" in n]
    print(kern)
    assert int(kern["ScratchSize"]) == 0
    assert int(kern["VGPRs Spill"]) == 0
    assert int(kern["VGPRs"]) <= 128
