"""The expert opponent's rules header (muzero.jl_amd/csrc/mz_expert_rules.h, the
code mz_expert_move runs per lane) as a stand-alone CPU program under
AddressSanitizer + UBSan (tests/sanitize/expert_rules_main.cpp): its scores
equal the Python mirror's on the random-play and hand-made positions, and
inconsistent boards are rejected, with no sanitizer report.  Nothing loaded
into Python runs under a sanitizer."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import expert_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sanitize", "expert_rules_main.cpp")


def test_rules_header_matches_mirror_sanitizer_clean(tmp_path):
    from muzero_jl_amd.games.expert import expert_scores
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "expert_rules_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True)
    lines, want = [], []
    for env, name in enumerate(xc.NAMES):
        cases = [(b, p, d) for d in xc.DEPTHS[name] for b, p in xc.random_positions(name) + xc.HAND[name]]
        if name == "connect4":
            cases += [(b, p, 6) for b, p in xc.random_positions(name)[:3]]
            cases += [(*xc.C4_LAST, 9)]                                  # the depth exceeds what is left
        for b, p, d in cases:
            lines.append(f"{env} {p} {d} {''.join(str(int(x)) for x in b)}")
            want.append(" ".join(str(int(s)) for s in expert_scores(name, b, p, d)))
        good = xc.HAND[name][0][0]
        for bad in xc.bad_boards(name):
            lines.append(f"{env} 1 3 {''.join(str(int(x)) for x in bad)}")
            want.append("rejected")
        for p, d, planes in ((0, 3, good), (3, 3, good), (1, 0, good), (1, 10, good), (1, 3, good[:-1])):
            lines.append(f"{env} {p} {d} {''.join(str(int(x)) for x in planes)}")
            want.append("rejected")
    lines.append("2 1 3 " + "0" * 27)                                    # not a board env
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
    assert np.sum([w == "rejected" for w in want]) == 15
