"""The rules-MCTS opponent's header (muzero.jl_amd/csrc/mz_mcts_rules.h: the
edge score and the rollout mz_mcts_move runs per lane, and the serial
mcts_root_stats) as a stand-alone CPU program under AddressSanitizer + UBSan
(tests/sanitize/mcts_rules_main.cpp): its n / w equal the Python mirror's on
the shared positions at every (S, R) setting, and inconsistent boards are
rejected, with no sanitizer report.  Nothing loaded into Python runs under a
sanitizer."""
import os
import shutil
import subprocess

import pytest

import mcts_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sanitize", "mcts_rules_main.cpp")


def _planes(b):
    return "".join(str(int(x)) for x in b)


def test_mcts_header_matches_mirror_sanitizer_clean(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "mcts_rules_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    lines, want = [], []
    for env, name in enumerate(mc.NAMES):
        for S, R in mc.SETTINGS:
            for k, (b, p) in enumerate(mc.positions(name)):
                ident, step = 3 + k, 5 + S                               # distinct Philox keys per case
                lines.append(f"{env} {p} {S} {R} {mc.SEED} {ident} {step} {_planes(b)}")
                n, w = mc.mirror(name, (b, p), S, R, ident, step)
                want.append(" ".join(str(int(x)) for x in list(n) + list(w)))
        good = mc.HAND[name][0][0]
        for bad in mc.xc.bad_boards(name):
            lines.append(f"{env} 1 8 4 {mc.SEED} 0 0 {_planes(bad)}")
            want.append("rejected")
        for p, S, R, planes in ((0, 8, 4, good), (3, 8, 4, good), (1, 0, 4, good), (1, 1025, 4, good), (1, 8, 0, good),
                                (1, 8, 65, good), (1, 8, 4, good[:-1])):
            lines.append(f"{env} {p} {S} {R} {mc.SEED} 0 0 {_planes(planes)}")
            want.append("rejected")
    lines.append(f"2 1 8 4 {mc.SEED} 0 0 " + "0" * 27)                   # not a board env
    want.append("rejected")
    path = tmp_path / "positions.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(want) and f"{len(want)} positions" in r.stderr
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, [(lines[i], got[i], want[i]) for i in bad[:5]]
    assert sum(w == "rejected" for w in want) == 19
