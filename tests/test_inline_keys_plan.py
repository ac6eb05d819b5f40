"""The inline-key form's launch plan (minbft_amd/csrc/verify_plan.h,
verify_keys_plan): where s^-1 comes from, the grid's threads and its block cap
-- plain C++, driven through the stand-alone program
tests/inline_keys_plan_check (built by __graft_entry__.build() from
tests/csrc/inline_keys_plan_check.cpp) and compared with a model written here.
No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "inline_keys_plan_check.cpp")
HIPCC = "/opt/rocm/bin/hipcc"

SIZES = [1, 63, 64, 65, 255, 256, 257, 4096, 4097, 1 << 20, 1 << 28]


@pytest.fixture(scope="module")
def prog():
    import __graft_entry__ as ge
    return ge.build_inline_keys_plan_check()


def run(prog, lines):
    p = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    return p.stdout.split("\n")[:-1]


def model(n, lane_inv_max, ncu, bpc):
    """One item per lane in whole blocks of 256; the grid is capped at bpc
    blocks per CU (grid-stride beyond); the lane inverts s itself up to
    lane_inv_max items, the batch's planes serve above."""
    want = -(-n // 256) if n > 0 else 0
    return int(n <= lane_inv_max), 256 * want, min(want, max(ncu, 1) * bpc)


def check(prog):
    bpc = int(run(prog, ["bpc"])[0])
    assert bpc == 2  # the kernel's occupancy: 2 waves a SIMD, 256-thread blocks
    cases = [(n, lim, ncu) for n in SIZES for lim in (4096, 0, 100, 1 << 40) for ncu in (256, 1, 8, 304)]
    cases += [(0, 4096, 256), (4096, 4095, 256), (5510, 4096, 256), (4160, 4096, 256), (1 << 28, 4096, 0)]
    out = run(prog, [f"plan {n} {lim} {ncu}" for n, lim, ncu in cases])
    assert len(out) == len(cases)
    for (n, lim, ncu), o in zip(cases, out):
        got = tuple(int(x) for x in o.split())
        assert got == model(n, lim, ncu, bpc), (n, lim, ncu, got)
        lane, threads, blocks = got
        # every item has a thread of the uncapped grid; the capped grid is never empty for n > 0,
        # and nothing overflows 32-bit grid dimensions
        assert threads >= n and threads - n < 256 and threads % 256 == 0
        assert (blocks >= 1) == (n > 0) and blocks * 256 <= threads and blocks < 1 << 31


def test_plan_sizes(prog):
    check(prog)
    # the default rule at the sizes the GPU tests run (MBFT_LANE_INV_MAX 4,096, 256 CUs)
    out = run(prog, [f"plan {n} 4096 256" for n in SIZES])
    assert [o.split()[0] for o in out] == ["1"] * 8 + ["0"] * 3
    assert [int(o.split()[2]) for o in out] == [1, 1, 1, 1, 1, 1, 2, 16, 17, 512, 512]
    assert int(out[-1].split()[1]) == 1 << 28


def test_plan_under_sanitizers(tmp_path):
    """The same stand-alone program built with AddressSanitizer and UBSan and
    run as a program over the same cases."""
    exe = str(tmp_path / "inline_keys_plan_check_san")
    # (host code only: the sanitizers are named for the host side of the compile and no GPU code is built)
    p = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-Xarch_host", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    check(exe)
