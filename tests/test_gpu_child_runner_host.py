"""tests/_gpu_child.py, the runner every GPU test starts its processes with, driven by stub scripts on the CPU: what
comes back, what a failure message holds, that a time limit leaves no process behind, and that nothing is started after
trouble.  The stubs import json, os, sys and time only.  The latch is set and cleared through monkeypatch alone, so a
whole-suite run keeps its own."""
import json
import os
import sys
import time

import pytest

import _gpu_child
from _gpu_child import child_main, run, run_case, run_ranks

# CASE OUT.json [ARG ...]: leaves a marker beside itself, writes what it was given
OK = """import json, os, sys
case, out, *args = sys.argv[1:]
open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ran"), "w").close()
json.dump({"case": case, "args": args, "cwd": os.getcwd()}, open(out, "w"))
"""
# CASE OUT.json STATUS: prints, then a plain exit with that status
EXIT = """import sys
print("stub output before the exit")
sys.exit(int(sys.argv[3]))
"""
# writes its pid beside itself, then sleeps; as rank 0 of several it exits at once instead
SLEEP = """import os, sys, time
here = os.path.dirname(os.path.abspath(__file__))
open(os.path.join(here, "pid" + os.environ.get("RANK", "")), "w").write(str(os.getpid()))
if os.environ.get("RANK") == "0":
    sys.exit(0)
time.sleep(30)
"""
FAULT = """import sys
print("HIP error: an illegal memory access was encountered")
sys.exit(1)
"""


@pytest.fixture(autouse=True)
def latch(monkeypatch):
    monkeypatch.setattr(_gpu_child, "LATCH", None)


def stub(tmp_path, name, text):
    path = tmp_path / name
    path.write_text(text)
    return str(path)


def gone(pid):
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return True
    return False


def test_a_case_returns_the_json_the_child_wrote(tmp_path):
    ok = stub(tmp_path, "ok.py", OK)
    r = run_case(ok, "shape", "h32", tmp_path=tmp_path, timeout=30)
    assert r == {"case": "shape", "args": ["h32"], "cwd": _gpu_child.ROOT}
    assert (tmp_path / "shape_h32.json").exists() and (tmp_path / "ran").exists()
    assert run_case(ok, "bitid", tmp_path=tmp_path, timeout=30)["args"] == [] and (tmp_path / "bitid.json").exists()
    assert run_case(ok, "mem", "train", tmp_path=tmp_path, timeout=30)["args"] == ["train"] and (tmp_path / "mem_train.json").exists()
    assert _gpu_child.LATCH is None


def test_an_ordinary_failure_shows_the_output_and_sets_no_latch(tmp_path):
    with pytest.raises(AssertionError) as e:
        run_case(stub(tmp_path, "exit.py", EXIT), "x", "3", tmp_path=tmp_path, timeout=30)
    assert "stub output before the exit" in str(e.value) and "[3]" in str(e.value)
    assert _gpu_child.LATCH is None
    assert run([sys.executable, "-c", "print('still runs')"], timeout=30) == "still runs\n"


def test_run_keeps_stdout_apart_on_request():
    prog = "import sys; print('{\"a\": 1}'); print('noise', file=sys.stderr)"
    assert json.loads(run([sys.executable, "-c", prog], timeout=30, split=True)) == {"a": 1}
    assert "noise" in run([sys.executable, "-c", prog], timeout=30)


def test_the_time_limit_kills_the_child_and_nothing_starts_afterwards(tmp_path):
    ok = stub(tmp_path, "ok.py", OK)
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match="time limit"):
        run_case(stub(tmp_path, "sleep.py", SLEEP), "x", tmp_path=tmp_path, timeout=1)
    assert time.monotonic() - t0 < 10
    assert gone(int((tmp_path / "pid").read_text()))
    assert "sleep.py" in _gpu_child.LATCH and "time limit" in _gpu_child.LATCH
    for call in (lambda: run_case(ok, "bitid", tmp_path=tmp_path, timeout=30),
                 lambda: run([sys.executable, ok, "bitid", str(tmp_path / "o.json")], timeout=30),
                 lambda: run_ranks([sys.executable, ok, "bitid", str(tmp_path / "o.json")], [None, None], timeout=30)):
        with pytest.raises(AssertionError, match="sleep.py") as e:
            call()
        assert "not started" in str(e.value)
    assert not (tmp_path / "ran").exists()


@pytest.mark.parametrize("status", [124, 134, 137, 139])
def test_a_status_that_means_trouble_sets_the_latch(tmp_path, status):
    """a plain sys.exit(status) of a CPU process: no signal is raised"""
    with pytest.raises(AssertionError):
        run_case(stub(tmp_path, "exit.py", EXIT), "x", str(status), tmp_path=tmp_path, timeout=30)
    assert str(status) in _gpu_child.LATCH
    with pytest.raises(AssertionError, match="not started"):
        run_case(stub(tmp_path, "ok.py", OK), "bitid", tmp_path=tmp_path, timeout=30)
    assert not (tmp_path / "ran").exists()


def test_a_memory_fault_in_the_output_sets_the_latch(tmp_path):
    with pytest.raises(AssertionError):
        run([sys.executable, stub(tmp_path, "fault.py", FAULT)], timeout=30)
    assert _gpu_child.LATCH is not None


def test_ranks_are_all_gone_after_the_limit(tmp_path):
    sleep = stub(tmp_path, "sleep.py", SLEEP)
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match="time limit"):
        run_ranks([sys.executable, sleep], [dict(os.environ, RANK=str(r)) for r in range(2)], timeout=1)
    assert time.monotonic() - t0 < 10
    assert gone(int((tmp_path / "pid0").read_text())) and gone(int((tmp_path / "pid1").read_text()))
    assert "rank 1" in _gpu_child.LATCH


def test_a_failed_rank_ends_the_others_without_the_latch(tmp_path):
    prog = stub(tmp_path, "ranks.py", SLEEP.replace("sys.exit(0)", "sys.exit(3)"))
    t0 = time.monotonic()
    with pytest.raises(AssertionError, match="exit status"):
        run_ranks([sys.executable, prog], [dict(os.environ, RANK=str(r)) for r in range(2)], timeout=20)
    assert time.monotonic() - t0 < 10
    pid1 = tmp_path / "pid1"                   # (rank 1 may have been killed before it wrote its pid)
    assert not (pid1.exists() and pid1.read_text()) or gone(int(pid1.read_text()))
    assert _gpu_child.LATCH is None


def test_ranks_return_their_outputs(tmp_path):
    outs = run_ranks([sys.executable, "-c", "import os; print('rank', os.environ['RANK'])"],
                     [dict(os.environ, RANK=str(r)) for r in range(2)], timeout=30, cwd=tmp_path)
    assert outs == ["rank 0\n", "rank 1\n"]


def test_child_main_argument_convention(tmp_path, capsys):
    """CASE OUT.json [ARG ...]; a case whose first parameter is `workdir` gets OUT.json's directory"""
    cases = {"plain": lambda: {"got": []}, "shape": lambda tag: {"got": [tag]}, "mem": lambda kind: {"got": [kind]}}

    def case_e2e(workdir):
        return {"got": [workdir]}

    def case_fit(workdir, tag):
        return {"got": [workdir, tag]}
    cases.update(e2e=case_e2e, fit=case_fit)
    for argv, want in ((["plain"], []), (["shape", "h32"], ["h32"]), (["mem", "train"], ["train"]),
                       (["e2e"], [str(tmp_path)]), (["fit", "x"], [str(tmp_path), "x"])):
        out = tmp_path / ("_".join(argv) + ".json")
        child_main(cases, argv=[argv[0], str(out)] + argv[1:])
        assert json.load(open(out)) == {"got": want}
        assert json.loads(capsys.readouterr().out) == {"got": want}
    child_main({"long": lambda: {"k": "v" * 10000}}, argv=["long", str(tmp_path / "long.json")])
    assert len(capsys.readouterr().out) == 6001 and len(json.load(open(tmp_path / "long.json"))["k"]) == 10000


def test_a_child_whose_own_child_ended_in_trouble_exits_with_a_status_that_means_trouble(tmp_path, monkeypatch):
    def case_fit():
        monkeypatch.setattr(_gpu_child, "LATCH", "fit: time limit of 400 s")       # as run() inside the case would have
        raise AssertionError("fit: killed at its time limit")
    with pytest.raises(SystemExit) as e:
        child_main({"fit": case_fit}, argv=["fit", str(tmp_path / "fit.json")])
    assert e.value.code in _gpu_child.TROUBLE_STATUS and not (tmp_path / "fit.json").exists()
