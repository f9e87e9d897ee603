"""CPU: the speculation tuner's rules (csrc/spec_tuner.h) played frame by frame by tests/spec_tuner_driver.cpp, a stand-alone program built
with the address and undefined-behaviour sanitizers.  Both schedules render the same pixels, so only this sees a wrong decision.

Timing model: a bracketed frame's timing is delivered before the next frame's decision; every speculated frame times `s` ms, every plain
frame `p` ms.  The expected traces are phase run-lengths over 1-based frame numbers, derived from the rules as they were when they still
lay between the event calls of gsx_frame.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgpu_3dgs_viewer_app_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spec_tuner") / "spec_tuner_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "spec_tuner_driver.cpp"), "-o", exe])
    return exe


def play(driver, script):
    """-> (frames: list of dicts in frame order, states: list of dicts, one per `state` command)"""
    r = subprocess.run([driver], input=script, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr  # (a sanitizer report)
    frames, states = [], []
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "state":
            states.append(dict(zip(("len_spec", "len_plain", "n_spec", "n_plain", "probe_pending", "left"), map(int, w[1:]))))
        else:
            frames.append(dict(no=int(w[0]), phase=w[1], speculates=bool(int(w[2])), bracketed=bool(int(w[3])), probe=bool(int(w[4])),
                               must_wait=bool(int(w[5])), windows=bool(int(w[6]))))
    return frames, states


def runs(frames):
    """phase run-lengths: [(first frame, last frame, phase)]"""
    out = []
    for f in frames:
        if out and out[-1][2] == f["phase"] and out[-1][1] + 1 == f["no"]:
            out[-1][1] = f["no"]
        else:
            out.append([f["no"], f["no"], f["phase"]])
    return [tuple(r) for r in out]


SPECULATING = {"SPEC", "PROBE_SPEC", "SETTLE_SPEC"}


def check_common(frames):
    """what holds on every trace: numbering, which phases speculate, which frames are bracketed"""
    assert [f["no"] for f in frames] == list(range(frames[0]["no"], frames[0]["no"] + len(frames)))
    first_of_run = {r[0] for r in runs(frames)}
    for f in frames:
        assert f["speculates"] == (f["phase"] in SPECULATING), f
        if f["phase"].startswith("PROBE"):  # the first frame of a probe is not bracketed, the other four are, as probe frames
            assert f["bracketed"] == (f["no"] not in first_of_run) and f["probe"] == f["bracketed"], f
        else:  # exactly the frames whose number is a multiple of 4
            assert f["bracketed"] == (f["no"] % 4 == 0) and not f["probe"], f


def test_speculation_pays_clearly(driver):
    frames, states = play(driver, "times 1.0 2.0\nframes 1500 deliver\nstate\n")
    check_common(frames)
    assert frames[0]["no"] == 1
    assert runs(frames) == [(1, 32, "SPEC"), (33, 37, "PROBE_PLAIN"), (38, 38, "SETTLE_SPEC"),
                            (39, 294, "SPEC"), (295, 299, "PROBE_PLAIN"), (300, 300, "SETTLE_SPEC"),
                            (301, 1324, "SPEC"), (1325, 1329, "PROBE_PLAIN"), (1330, 1330, "SETTLE_SPEC"), (1331, 1500, "SPEC")]
    assert states[0]["len_spec"] == 2048 and states[0]["len_plain"] == 64
    assert not any(f["must_wait"] for f in frames), "every timing was in before its decision"


def test_plain_pays_clearly(driver):
    frames, states = play(driver, "times 2.0 1.0\nlanes 2\nframes 1500 deliver\nstate\n")
    check_common(frames)
    assert runs(frames) == [(1, 32, "SPEC"), (33, 37, "PROBE_PLAIN"), (38, 38, "SETTLE_SPEC"),
                            (39, 102, "PLAIN"), (103, 107, "PROBE_SPEC"), (108, 108, "SETTLE_PLAIN"),
                            (109, 364, "PLAIN"), (365, 369, "PROBE_SPEC"), (370, 370, "SETTLE_PLAIN"),
                            (371, 1394, "PLAIN"), (1395, 1399, "PROBE_SPEC"), (1400, 1400, "SETTLE_PLAIN"), (1401, 1500, "PLAIN")]
    assert states[0]["len_plain"] == 2048 and states[0]["len_spec"] == 64
    # windows in the plain phase of frames 39-102: only its last L frames must leave any (every lane needs ITS windows for the probe that
    # follows).  The rule reads `left` after the frame's own decrement (do_preprocess asked it behind tuner_wants_speculation, and still
    # does): frame k of this phase has left = 102 - k, so `left >= 2` holds through frame 100 and `left >= 1` through frame 101.
    # (The issue that asked for this test put the two-lane boundary at frame 101, "left >= 2 holds through frame 101": that is the value
    # before the decrement, which the rule never saw — with it the first lane's probe frame would find no windows of its own.)
    by_no = {f["no"]: f for f in frames}
    assert not any(by_no[k]["windows"] for k in range(39, 101))
    assert by_no[101]["windows"] and by_no[102]["windows"]
    assert all(f["windows"] for f in frames if f["phase"] != "PLAIN")
    one_lane, _ = play(driver, "times 2.0 1.0\nlanes 1\nframes 110 deliver\n")
    by_no = {f["no"]: f for f in one_lane}
    assert not any(by_no[k]["windows"] for k in range(39, 102))
    assert by_no[102]["windows"]


def test_close_verdict_doubles_the_phase(driver):
    frames, _ = play(driver, "times 1.0 1.02\nframes 1000 deliver\n")
    check_common(frames)
    assert runs(frames) == [(1, 32, "SPEC"), (33, 37, "PROBE_PLAIN"), (38, 38, "SETTLE_SPEC"),
                            (39, 166, "SPEC"), (167, 171, "PROBE_PLAIN"), (172, 172, "SETTLE_SPEC"),
                            (173, 428, "SPEC"), (429, 433, "PROBE_PLAIN"), (434, 434, "SETTLE_SPEC"),
                            (435, 946, "SPEC"), (947, 951, "PROBE_PLAIN"), (952, 952, "SETTLE_SPEC"), (953, 1000, "SPEC")]


def test_withheld_timings_make_the_host_wait_eight_frames_behind_the_probe(driver):
    frames, _ = play(driver, "times 1.0 2.0\nframes 320 withhold\n")
    check_common(frames)
    assert [f["no"] for f in frames if f["must_wait"]][0] == 46, "first at frame 46, nowhere before it"
    assert runs(frames)[:5] == [(1, 32, "SPEC"), (33, 37, "PROBE_PLAIN"), (38, 45, "SETTLE_SPEC"), (46, 301, "SPEC"), (302, 306, "PROBE_PLAIN")]


def test_a_dropped_probe_bracket_is_not_waited_for(driver):
    # frame 33 opens the probe (not bracketed); frame 34's bracket stays open and is dropped; 35-37 are withheld
    frames, states = play(driver, "times 1.0 2.0\nframes 33 deliver\nframes 1 open\nstate\ndrop\nstate\nframes 5 withhold\nstate\nflush\nstate\n"
                                  "frames 1 withhold\n")
    check_common(frames)
    assert [s["probe_pending"] for s in states] == [1, 0, 3, 0]
    assert runs(frames) == [(1, 32, "SPEC"), (33, 37, "PROBE_PLAIN"), (38, 39, "SETTLE_SPEC"), (40, 40, "SPEC")]
    assert not any(f["must_wait"] for f in frames)
    assert states[3]["n_plain"] == 3, "three probe timings fed the decision, the dropped one none"


def test_reset_mid_cycle_starts_over(driver):
    frames, states = play(driver, "times 1.0 2.0\nframes 35 withhold\nreset\nstate\nframes 40 deliver\n")
    assert runs(frames) == [(1, 32, "SPEC"), (33, 35, "PROBE_PLAIN"), (36, 67, "SPEC"), (68, 72, "PROBE_PLAIN"), (73, 73, "SETTLE_SPEC"),
                            (74, 75, "SPEC")]
    s = states[0]
    assert (s["n_spec"], s["n_plain"], s["probe_pending"], s["left"], s["len_spec"], s["len_plain"]) == (0, 0, 0, 32, 64, 64)


def test_the_rules_stand_alone():
    """spec_tuner.h: the standard library only; the driver: that header only"""
    import re
    with open(os.path.join(CSRC, "spec_tuner.h")) as f:
        inc = re.findall(r'#include\s+([<"][^>"]+[>"])', f.read())
    assert inc and all(i.startswith("<") and "hip" not in i for i in inc), inc
    with open(os.path.join(ROOT, "tests", "spec_tuner_driver.cpp")) as f:
        inc = [i for i in re.findall(r'#include\s+([<"][^>"]+[>"])', f.read()) if i.startswith('"')]
    assert inc == ['"spec_tuner.h"']
