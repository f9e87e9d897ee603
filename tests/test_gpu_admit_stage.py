"""GPU: the admission stage alone (kernels_admit.hip, window_scan.h, the window pyramid) against a host compaction, at
the counts and admitted sets where its five compaction kernels change path and whole frames only arrive by accident:
either side of the tiling switch of k_admit_compact (4 194 241 Gaussians), tiles that take 1, 2 and 8 LDS pages, the
second super-tile of k_admit_scan (above 10 485 760), the hand-over of the histogram and key range to
launch_bucket_sort(hist_done = true), one workspace reused by launches of different tilings, tails that are no multiple
of 64 / 256, and the window predicate — exact windows with and without a gate, and the conservative pyramid, which must
never refuse what an exact window admits.  tools/check_admit (built by __graft_entry__.build()) holds the cases and the
reference; every comparison is exact.  One child process per group, with a time limit: a look-back that hangs is a
failure, not a stuck test run — and after a child that died or hung nothing more is started on the GPU from here."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "check_admit")

GROUPS = ["small", "threshold", "superscan", "pages", "handover", "reuse", "windows", "pyramid"]

_dead = []  # why the remaining groups do not start another GPU process


@pytest.mark.parametrize("group", GROUPS)
def test_admit_stage(group):
    if _dead:
        pytest.skip(_dead[0])
    assert os.path.exists(EXE), "tools/check_admit missing: run __graft_entry__.build()"
    try:
        p = subprocess.run([EXE, group], capture_output=True, text=True, timeout=60)
    except subprocess.TimeoutExpired as e:
        _dead.append(f"tools/check_admit {group} did not end within 60 s: no further GPU process from this file")
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.fail(_dead[0] + "\n" + out[-1500:])
    if p.returncode < 0 or p.returncode == 134:
        _dead.append(f"tools/check_admit {group} ended by signal / abort (status {p.returncode}): no further GPU process from this file")
    elif p.returncode == 2:  # the checker's status for a HIP error (a fault is one): the device may be in no state to go on
        _dead.append(f"tools/check_admit {group} stopped at a HIP error: no further GPU process from this file")
    tail = p.stdout[-2500:] + p.stderr[-500:]
    assert p.returncode == 0, tail
    assert f"check_admit {group}: " in p.stdout and " cases, 0 mismatches\n" in p.stdout, tail
    # the checker's own test ran: each of the three corruptions of a reference was reported by its comparer
    assert "self-test: swapped pairs reported, index off by one reported, total one short reported" in p.stdout, p.stdout[:600]
