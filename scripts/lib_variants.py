#!/usr/bin/env python3
"""One script under several builds of the library, two interleaved rounds (a b c a b c) in a fresh process per build, so that
no build owns the warm end of the run:

    python3 scripts/lib_variants.py [--limit SECONDS] LIB... -- SCRIPT ARGS...

LIB is a path for SIREN_FIT_LIB; the word `product` unsets it (the library of this tree).  SCRIPT is a file under scripts/:
`-- kbench.py 4096` gives a line per build with every kernel above 0.05 ms (k_fwd, k_bwd_hidden, ...), `-- kbench.py 2048 512
8 12` the wide path at format 12.  Each run is a pass of profile_passes.run_passes: under `timeout -k 10 LIMIT` (default 180
s), stderr shown, and the first run that fails ends the whole comparison with its status."""
import os
import sys

from profile_passes import ROOT, run_passes


def main(args):
    limit = 180
    if args[:1] == ["--limit"]:
        limit, args = int(args[1]), args[2:]
    if "--" not in args or not args.index("--") or args[-1] == "--":
        sys.exit(__doc__.split("\n\n")[1])
    libs, (script, *script_args) = args[:args.index("--")], args[args.index("--") + 1:]
    base = {k: v for k, v in os.environ.items() if k != "SIREN_FIT_LIB"}
    passes = [dict(name=f"round {r} {lib}", limit=limit, cwd=ROOT, env=base if lib == "product" else {**base, "SIREN_FIT_LIB": lib},
                   argv=[sys.executable, os.path.join(ROOT, "scripts", script), *script_args])
              for r in (1, 2) for lib in libs]
    return run_passes(passes)


if __name__ == "__main__":
    sys.exit(min(abs(main(sys.argv[1:])), 255))
