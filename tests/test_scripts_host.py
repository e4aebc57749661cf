"""scripts/ on the CPU: every script compiles, the README table and the directory agree, the profiler driver's passes are the
recorded ones, and its runner starts nothing after a pass that failed.  No GPU, no GPU process."""
import json
import os
import py_compile
import re
import shlex
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")


def _files():
    """every file under scripts/ but caches and the probes' own binaries (built in place, not kept), relative to it"""
    return sorted(os.path.relpath(os.path.join(base, n), SCRIPTS) for base, _, names in os.walk(SCRIPTS)
                  for n in names if n.endswith((".py", ".sh", ".hip", ".md")))


def test_scripts_compile_and_common_leaves_the_device_alone(tmp_path):
    for f in _files():
        if f.endswith(".py"):
            py_compile.compile(os.path.join(SCRIPTS, f), cfile=str(tmp_path / "out.pyc"), doraise=True)
    code = ("import sys, torch; import _common; assert not torch.cuda.is_initialized(); "
            "assert callable(_common.timing_engine) and callable(_common.alternate); "
            "import _gpu_fixtures; assert not torch.cuda.is_initialized()")
    r = subprocess.run([sys.executable, "-c", code], cwd=SCRIPTS, capture_output=True, text=True, timeout=120,
                       env={**os.environ, "HIP_VISIBLE_DEVICES": "", "PYTHONPATH": SCRIPTS})
    assert r.returncode == 0, r.stderr


def test_readme_lists_exactly_the_files_present():
    text = open(os.path.join(SCRIPTS, "README.md")).read()
    rows = [line.split("|")[1] for line in text.splitlines() if line.startswith("| `")]
    named = {m for cell in rows for m in re.findall(r"`((?:probes/)?[\w.]+\.(?:py|sh|hip|md))\b", cell)} | {"README.md"}
    present = set(_files())
    assert named - present == set(), "README.md names files that are not there"
    assert present - named == set(), "files without a row in README.md"


@pytest.mark.parametrize("preset", ["collect", "wide", "sq", "lds", "ea"])
def test_profile_passes_dry_run_is_the_recorded_plan(preset):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "profile_passes_plan.json")))[preset]
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, "profile_passes.py"), "--dry-run", "--out", os.path.join(ROOT, "OUT"),
                        preset, "TAG"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = []
    for line in r.stdout.splitlines():
        argv = shlex.split(line)
        assert argv[:3] == ["timeout", "-k", "10"] and int(argv[3]) > 0, line
        argv = [a.replace(ROOT, "R") for a in argv[4:]]
        cut = argv.index("--") if "--" in argv else 0
        got.append({"rocprofv3": argv[:cut], "workload": argv[cut + 1 if cut else 0:]})
    assert got == want


@pytest.mark.parametrize("failing", [*([sys.executable, "-c", f"import sys; sys.exit({s})"] for s in (1, 124, 134, 137, 139)),
                                     ["sleep", "5"]], ids=["1", "124", "134", "137", "139", "limit"])
def test_runner_starts_nothing_after_a_failed_pass(failing, tmp_path, capfd):
    sys.path.insert(0, SCRIPTS)
    try:
        from profile_passes import run_passes
    finally:
        sys.path.remove(SCRIPTS)
    marker = tmp_path / "marker"
    status = run_passes([dict(name="first", argv=["true"], limit=30),
                         dict(name="the-failing-one", argv=failing, limit=1 if failing[0] == "sleep" else 30),
                         dict(name="marker", argv=["touch", str(marker)], limit=30)])
    want = 124 if failing[0] == "sleep" else int(re.search(r"exit\((\d+)\)", failing[2]).group(1))
    assert status == want and status != 0
    assert not marker.exists()
    err = capfd.readouterr().err
    assert f"pass the-failing-one ended with status {want}" in err and "pass marker" not in err


def test_no_process_start_discards_stderr():
    bad = []
    for f in _files():
        for i, line in enumerate(open(os.path.join(SCRIPTS, f), errors="replace"), 1):
            if re.search(r"2>\s*/dev/null", line) and re.search(r"\b(python3?|rocprofv3)\b", line.split("2>")[0]):
                bad.append(f"{f}:{i}")
    assert not bad, bad
