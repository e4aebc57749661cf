"""The one place a GPU test starts a process: run_case for the tests/_*_child.py scripts, run for any other program,
run_ranks for several at once; child_main is what a child script ends with.  No torch here: a parent pays nothing to
import this.  Importing it puts the repository root and the package directory on sys.path, which is all the path setup
a child (run as a script, so tests/ is sys.path[0] already) needs.

Arguments of a child: CASE OUT.json [ARG ...].  The case function gets the ARGs as strings; a case whose first parameter
is called `workdir` gets the directory of OUT.json in front of them.

After trouble, nothing more is started: when a process started here ends at its time limit, by a signal, with status 124,
134, 137 or 139, or with a GPU memory fault in its output, LATCH names it and every later run_case / run / run_ranks of
this pytest process fails at once.  An ordinary non-zero exit (an exception or a failed assertion in a child) does not
set it."""
import inspect
import json
import os
import signal
import subprocess
import sys
import tempfile
import time

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, os.path.join(ROOT, "implicit-image-compression_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

TROUBLE_STATUS = (124, 134, 137, 139)          # timeout(1)'s two, abort, segmentation fault
MEMORY_FAULT = "an illegal memory access was encountered"
LATCH = None                                   # what ended in trouble first, once something has


def _run_all(argvs, envs, timeout, cwd, split):
    """Start every argv, wait for all of them under one limit and kill every process group still alive when the limit
    passes or one of them fails.  -> [(stdout, stderr)] as text (stderr is in stdout unless split)."""
    global LATCH
    what = " ".join(os.path.basename(a) if os.sep in a else a for a in argvs[0][:4])
    assert LATCH is None, f"not started ({what}): an earlier GPU process ended in trouble: {LATCH}"
    files = [(tempfile.TemporaryFile(), tempfile.TemporaryFile() if split else subprocess.STDOUT) for _ in argvs]
    procs = [subprocess.Popen(a, cwd=cwd, env=e, stdout=f[0], stderr=f[1], start_new_session=True)
             for a, e, f in zip(argvs, envs, files)]
    deadline = time.monotonic() + timeout
    status = [p.poll() for p in procs]         # None: still running
    while None in status and not any(status) and time.monotonic() < deadline:
        time.sleep(0.02)
        status = [p.poll() for p in procs]
    timed_out = None in status and not any(status)
    for p in procs:
        if p.returncode is None:
            try:
                os.killpg(p.pid, signal.SIGKILL)
            except ProcessLookupError:
                pass
        p.wait()
    outs = []
    for out, err in files:
        texts = []
        for f in (out, err):
            if f is not subprocess.STDOUT:
                f.seek(0)
                texts.append(f.read().decode(errors="replace"))
                f.close()
        outs.append((texts[0], texts[1] if split else ""))
    tail = "\n".join(o + e for o, e in outs)[-4000:]
    for i, rc in enumerate(status):
        if (rc is None and timed_out) or (rc is not None and (rc < 0 or rc in TROUBLE_STATUS)) or MEMORY_FAULT in "".join(outs[i]):
            how = f"time limit of {timeout} s" if rc is None else f"exit status {rc}"
            LATCH = LATCH or f"{what}{f' [rank {i}]' if len(procs) > 1 else ''}: {how}"
    assert not timed_out, f"{what}: killed at its time limit of {timeout} s\n{tail}"
    assert not any(status), f"{what}: exit status {status}\n{tail}"
    return outs


def run(argv, *, timeout, cwd=ROOT, env=None, split=False):
    """One program under `timeout`; asserts exit status 0 with the end of its output in the message.  -> its output:
    stdout and stderr together, or stdout alone with split=True"""
    return _run_all([list(argv)], [env], timeout, cwd, split)[0][0]


def run_ranks(argv, envs, *, timeout, cwd=ROOT):
    """One process of `argv` per environment, all under one time limit.  -> their outputs"""
    return [o for o, _ in _run_all([list(argv)] * len(envs), envs, timeout, cwd, False)]


def run_case(child, case, *args, tmp_path, timeout):
    """python tests/<child> CASE OUT.json ARGS... from the repository root -> the JSON the child wrote, which stays in
    tmp_path as <case>[_<arg>...].json"""
    out = os.path.join(str(tmp_path), "_".join((case,) + args) + ".json")
    run([sys.executable, os.path.join(TESTS, child), case, out, *args], timeout=timeout)
    with open(out) as f:
        return json.load(f)


def child_main(cases, argv=None):
    """What a child ends with: cases[CASE](*ARGS) -> OUT.json, and the start of it on stdout"""
    case, out, *args = sys.argv[1:] if argv is None else argv
    fn = cases[case]
    if next(iter(inspect.signature(fn).parameters), None) == "workdir":
        args.insert(0, os.path.dirname(os.path.abspath(out)))
    try:
        res = fn(*args)
    except BaseException:
        if LATCH is not None:                  # a process this child started ended in trouble: tell the parent's latch
            import traceback
            traceback.print_exc()
            sys.exit(124)
        raise
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res)[:6000])
