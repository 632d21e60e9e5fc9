"""bench.py with functional.CONV3X3_DGRAD set from outside it (the benchmark itself stays as it is), off and on alternating
in one call:
    python scripts/bench_conv3x3_dgrad_switch.py pairs 4 [all] --gpus 1 --steps 12 --warmup 4
runs `off`, `on`, `off`, `on`, ... (4 pairs), each a fresh child process of
    python scripts/bench_conv3x3_dgrad_switch.py on|off [all] --gpus 1 --steps 12 --warmup 4
(under a time limit of its own; a child that fails or runs into it ends the call) and prints each child's JSON result line
behind its label.  `all` also turns CONV3X3_FWD, CONV3X3_WGRAD and STEM_WGRAD on, on
both sides.  The whole-step table of profiles/conv3x3_dgrad.md is the output of the `pairs` form."""
import os
import runpy
import subprocess
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if sys.argv[1] == "pairs":
    pairs, rest = int(sys.argv[2]), sys.argv[3:]
    for i in range(pairs):
        for side in ("off", "on"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), side] + rest, check=True, stdout=subprocess.PIPE,
                                 text=True, timeout=600).stdout       # (a child that fails or hangs ends the call)
            lines = [ln for ln in out.splitlines() if ln.startswith("{")]
            print(f"pair {i} {side}: {lines[-1] if lines else out[-400:]}", flush=True)
else:
    sys.path.insert(0, root)
    os.chdir(root)
    import mrla_amd.functional as Fm  # noqa: E402

    Fm.CONV3X3_DGRAD = sys.argv[1] == "on"
    rest = sys.argv[2:]
    if rest and rest[0] == "all":
        Fm.CONV3X3_FWD = Fm.CONV3X3_WGRAD = Fm.STEM_WGRAD = True
        rest = rest[1:]
    sys.argv = ["bench.py"] + rest
    runpy.run_path(os.path.join(root, "bench.py"), run_name="__main__")
