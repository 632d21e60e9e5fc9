"""bench.py with functional.STEM_WGRAD set from outside it (the benchmark itself stays as it is):
    python scripts/bench_stem_switch.py on|off|both --gpus 1 --steps 12 --warmup 4
`both` turns functional.CONV3X3_WGRAD on as well (mrla_amd.reproducible_gradients()).  The whole-step table of
profiles/stem_wgrad.md alternates `off` and `on` runs of this command."""
import os
import runpy
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
os.chdir(root)
import mrla_amd.functional as Fm  # noqa: E402

Fm.STEM_WGRAD = sys.argv[1] in ("on", "both")
Fm.CONV3X3_WGRAD = sys.argv[1] == "both"
sys.argv = ["bench.py"] + sys.argv[2:]
runpy.run_path(os.path.join(root, "bench.py"), run_name="__main__")
