"""Write the launch-trace golden: every scenario of tests/launch_trace_cases.py in its three modes, on the GPU.

    python scripts/record_launch_trace.py [--out tests/golden/launch_trace.json] [--only NAME ...]

The golden pins what mrla_amd/functional.py asks of the C ABI; it is recorded from the commit whose launches are to be
kept (for a refactor of functional.py: the parent commit, with the same library build) and committed.  With --check the
file is not written: the traces are compared with the one that is there and the first difference of each is printed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "launch_trace.json"))
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    from tests import launch_trace_cases as ltc
    traces, failed = {}, []
    for s in ltc.SCENARIOS:
        if args.only and s.name not in args.only:
            continue
        for mode in ltc.MODES:
            key = f"{s.name}/{mode}"
            try:
                traces[key] = ltc.trace(s, mode, strict=False)
            except Exception as e:      # (a scenario that does not run: reported below, the others are still recorded)
                failed.append(f"{key}: {type(e).__name__}: {e}")
                continue
            lacks = ltc.missing(s, mode, traces[key])
            if lacks:
                failed.append(f"{key}: the trace lacks {lacks}; it has {sorted({r[0] for r in traces[key]})}")
            print(f"{key}: {len(traces[key])} records", flush=True)
    if args.check:
        with open(args.out) as fh:
            golden = json.load(fh)
        bad = {k: d for k, d in ((k, ltc.first_difference(v, ltc.unpack(golden, k))) for k, v in traces.items()) if d}
        for k, d in bad.items():
            print(f"DIFFERS {k}: {d}")
        print(f"{len(traces) - len(bad)} of {len(traces)} traces equal the golden")
        print("\n".join(["FAILED " + f for f in failed]))
        return 1 if (bad or failed) else 0
    packed = ltc.pack(traces)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(packed, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{len(traces)} traces, {len(packed['table'])} distinct records -> {args.out} ({os.path.getsize(args.out)} bytes)")
    print("\n".join(["FAILED " + f for f in failed]))           # (a golden with such a scenario in it is not to be committed)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
