"""The signer kernels keep every lane secret in registers: sign_kernels.hip,
compiled for gfx950 with the flags of minbft_amd/build.py and
-Rpass-analysis=kernel-resource-usage, reports 0 bytes of scratch and 0 bytes
of LDS for k_sign_tags and k_usig_uis (the key, the nonce
and its inverse never land in memory).  A condition, not a measurement; the
VGPR count is printed, not asserted.  One device-only compile (about two
minutes); skipped without hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """{kernel name: {"scratch": bytes / lane, "lds": bytes / block, "vgprs": n}}"""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    from minbft_amd import build as b
    src = os.path.join(b.CSRC, "sign_kernels.hip")
    obj = str(tmp_path_factory.mktemp("sign_res") / "sign_kernels.o")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", *b.COMMON_FLAGS, "--offload-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    out, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("vgprs", r" VGPRs: (\d+)")):
            m = re.search(pat, line)
            if m and name is not None:
                out[name][key] = int(m.group(1))
    return out


@pytest.mark.parametrize("kernel", ["k_sign_tags", "k_usig_uis"])
def test_no_scratch_no_lds(usage, kernel):
    hits = [(nm, u) for nm, u in usage.items() if kernel in nm]
    assert len(hits) == 1, sorted(usage)
    nm, u = hits[0]
    print(nm, u)
    assert u["scratch"] == 0
    assert u["lds"] == 0
