"""The P-384 class's arithmetic on the host (minbft_amd/csrc/p384_fe.h,
p384_ecc.h) and its launch plan (verify_p384_plan,
verify_plan.h), through the stand-alone program tests/p384_host_check (built
by __graft_entry__.build() from tests/csrc/p384_host_check.cpp), against Python
integers (tests/p384_ops_util.py, tests/p384_ref.py): field operations on 0,
1, p - 1, p - 2, all-ones limbs and random elements, Montgomery round trips,
the scalar product, inverse and e mod N, the complete addition on (P, P),
(P, -P), (P, O), (O, P) and (O, O), the finish on an injected (X, Z) with
x = r + N, and the whole item function on every fixture vector.  The same
program is built again with AddressSanitizer and UBSan and run once.  No GPU."""
import importlib.util
import os
import subprocess

import pytest

import p384_ops_util as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "p384_host_check.cpp")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def prog():
    import __graft_entry__ as ge
    return ge.build_p384_host_check()


def run_file(prog, lines, tmp_path):
    """The vectors go through a file, as the program reads them."""
    path = tmp_path / "p384_vectors.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = p.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return out


def check_ops(prog, cases, tmp_path):
    out = run_file(prog, ["%s %s" % (op, " ".join("%x" % v for v in a)) for op, a in cases], tmp_path)
    for (op, a), line in zip(cases, out):
        got = [int(x, 16) for x in line.split()]
        assert len(got) == u.OPS[op][1]
        u.check(op, a, got)


def test_every_operation_against_python_integers(prog, tmp_path):
    cases = u.cases()
    assert {op for op, _ in cases} == set(u.OPS)
    assert u.finish_cases_cover() >= 4
    assert sum(op == "item" for op, _ in cases) >= 200
    check_ops(prog, cases, tmp_path)


def test_header_constants_are_the_generators():
    """The tables of p384_fe.h are what tools/p384_consts.py prints."""
    spec = importlib.util.spec_from_file_location("p384_consts", os.path.join(ROOT, "tools", "p384_consts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import re
    text = open(os.path.join(ROOT, "minbft_amd", "csrc", "p384_fe.h")).read()
    consts = mod.constants()
    assert (mod.P, mod.N, mod.B, mod.GX, mod.GY) == (u.P, u.N, u.o.B, u.o.GX, u.o.GY)
    for name, vals in consts.items():
        if name == "kN384INV":
            m = re.search(r"constexpr uint32_t kN384INV = (0x[0-9a-f]+)u;", text)
            assert m and int(m.group(1), 16) == vals[0]
            assert (u.N * vals[0] + 1) % (1 << 28) == 0
            continue
        m = re.search(r"P384_CONST uint32_t %s\[\w+\] = \{([^}]*)\};" % name, text)
        assert m, name
        got = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
        assert got == vals, name


def plan_model(n, ncu):
    """Whole blocks of 256, one block per CU at the most (the kernel's occupancy)."""
    want = 0 if n <= 0 else -(-n // 256)
    return want * 256, min(want, max(ncu, 1) * 1)


def test_plan_against_model(prog, tmp_path):
    ns = [0, 1, 255, 256, 257, 65535, 65536, 65537, 256 * 256, 256 * 256 + 1, 1 << 20, (1 << 28) - 1, 1 << 28, -5]
    ns += [256 * k + d for k in (1, 7, 255, 256, 257, 304) for d in (-1, 0, 1)]
    cus = [1, 8, 256, 304, 0]
    cases = [(n, c) for n in ns for c in cus]
    out = run_file(prog, ["plan %d %d" % nc for nc in cases], tmp_path)
    for nc, line in zip(cases, out):
        assert tuple(int(x) for x in line.split()) == plan_model(*nc), nc
    # every item has a lane within a whole number of passes, and the grid never passes the cap
    for (n, c), line in zip(cases, out):
        threads, blocks = (int(x) for x in line.split())
        assert threads >= n and threads % 256 == 0 and (n <= 0 or threads - n < 256)
        assert blocks <= max(c, 1) and (blocks > 0) == (n > 0)


def test_host_check_under_sanitizers(tmp_path):
    """The same stand-alone program built with AddressSanitizer and UBSan and
    run once over a cut of the vectors (every operation, fewer items)."""
    exe = str(tmp_path / "p384_host_check_san")
    # (host code only: the sanitizers are named for the host side of the compile and no GPU code is built)
    p = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-Xarch_host", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    seen, cut = {}, []
    for op, a in u.cases():
        seen[op] = seen.get(op, 0) + 1
        if seen[op] <= (6 if op in ("item", "shamir", "inv", "ninv", "finish", "u1u2") else 40):
            cut.append((op, a))
    assert {op for op, _ in cut} == set(u.OPS)
    check_ops(exe, cut, tmp_path)
    out = run_file(exe, ["plan 1000 256", "plan 0 256"], tmp_path)
    assert out == ["1024 4", "0 0"]
