"""bench.py with functional.STEM_WGRAD_F32 set from outside it (the benchmark itself stays as it is):
    python scripts/bench_stem_f32_switch.py on|off --gpus 1 --steps 12 --warmup 4 --autocast none --batch 64 --no-others
The whole-step table of profiles/stem_wgrad_f32.md alternates `off` and `on` runs of this command, each a fresh process."""
import os
import runpy
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
os.chdir(root)
import mrla_amd.functional as Fm  # noqa: E402

Fm.STEM_WGRAD_F32 = sys.argv[1] == "on"
sys.argv = ["bench.py"] + sys.argv[2:]
runpy.run_path(os.path.join(root, "bench.py"), run_name="__main__")
