"""The network-only player's header (muzero.jl_amd/csrc/mz_prior_rules.h: the
policy over the legal actions and the action, the scalar pieces mz_prior_fc /
mz_prior_pick run per lane and the serial mzp_row) as a stand-alone CPU program
under AddressSanitizer + UBSan (tests/sanitize/prior_rules_main.cpp): π and the
action equal the Python mirror's bit for bit on the shared cases, what mzp_row
refuses is rejected, and no sanitizer report appears.  Nothing loaded into
Python runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

import prior_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sanitize", "prior_rules_main.cpp")


def test_prior_header_matches_mirror_sanitizer_clean(tmp_path):
    from muzero_jl_amd.selfplay import prior_pick, prior_policy
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "prior_rules_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    dm = pc.OracleMath()
    lines, want = [], []
    for _, p, legal, T, r in pc.cases():
        lines.append(pc.case_line(p, legal, T, r))
        pi = prior_policy(p, legal)
        want.append(pc.result_line(prior_pick(pi, legal, T, r, dm), pi))
    _, p, legal = pc.rows()[0]
    none = [False] * len(p)
    for line in (pc.case_line(p, none, 1.0, 5),                      # no legal action
                 pc.case_line(p, legal, -1.0, 5),                    # T < 0
                 pc.case_line(p, legal, float("nan"), 5),            # T is NaN
                 pc.case_line(p, legal, 1.0, 5) + " 3f800000",       # one value too many
                 pc.case_line(p[:-1], legal, 1.0, 5),                # mask and p disagree
                 "0 3f800000 5 "):                                   # A = 0
        lines.append(line)
        want.append("rejected")
    path = tmp_path / "rows.txt"
    path.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(want) and f"{len(want)} rows" in r.stderr
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, [(lines[i], got[i], want[i]) for i in bad[:5]]
    assert sum(w == "rejected" for w in want) == 6
