"""Is mrla_conv3x3_wgrad of this build bit-equal to another build's (an older commit's libmrla_hip.so)?  A change to the
kernel's loader, schedule or registers that keeps the arithmetic order -- same steps, same k-steps, same nine taps -- must
leave `part` and `dw` bit for bit what they were, not merely inside the tests' bounds.  One process per library, then a
comparison (not a test: it needs the other build):

    python scripts/conv3x3_wgrad_against_build.py dump DIR/this
    MRLA_HIP_LIB=/path/to/other/libmrla_hip.so python scripts/conv3x3_wgrad_against_build.py dump DIR/other
    python scripts/conv3x3_wgrad_against_build.py compare DIR/this DIR/other

`dump` runs every shape of tests/test_conv3x3_wgrad_gpu.py and tests/test_conv3x3_wgrad_prefetch_gpu.py and the seven 3x3
convolutions of ResNet-50 at batch 256, in bf16 and fp16 with fp32 and 16-bit dw, on normal inputs from a seeded generator,
into NaN-filled buffers, and writes per case the number of elements of part and dw and their SHA-256; the first 2^20 elements
of each are kept as well, so that `compare` can count differing elements where a digest differs.  `compare` prints one line
per case and exits 1 unless every part and dw is equal."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEEP = 1 << 20
RESNET50 = [(256, c, c, h, h, s) for c, h, s in ((64, 56, 1), (128, 56, 2), (128, 28, 1), (256, 28, 2), (256, 14, 1), (512, 14, 2),
                                                (512, 7, 1))]


def shapes():
    from tests.test_conv3x3_wgrad_gpu import SHAPES as A
    from tests.test_conv3x3_wgrad_prefetch_gpu import SHAPES as B
    return list(A) + list(B) + RESNET50


def dump(out_dir):
    import torch

    from conv3x3_wgrad_kernel_times import own_entry_points
    from mrla_amd import _lib as L
    os.makedirs(out_dir, exist_ok=True)
    wgrad_rows, wgrad = own_entry_points()
    CL = torch.channels_last
    st = torch.cuda.current_stream().cuda_stream
    index = {}
    for i, (b, c, n, h, w, s) in enumerate(shapes()):
        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
        gen = torch.Generator(device="cuda").manual_seed(1000 + i)
        x32 = torch.randn(b, c, h, w, device="cuda", generator=gen)
        dy32 = torch.randn(b, n, ho, wo, device="cuda", generator=gen)
        for dname, dtype, dt in (("bf16", torch.bfloat16, L.BF16), ("f16", torch.float16, L.F16)):
            x, dy = x32.to(dtype).contiguous(memory_format=CL), dy32.to(dtype).contiguous(memory_format=CL)
            rows = wgrad_rows(b, c, n, h, w, s, dt)
            assert rows > 0, (b, c, n, h, w, s)
            for wname, dw_dtype, dwt in (("dw_f32", torch.float32, L.F32), ("dw_16", dtype, dt)):
                part = torch.full((rows, n, 9, c), float("nan"), device="cuda")
                dw = torch.full((n, 3, 3, c), float("nan"), dtype=dw_dtype, device="cuda")
                L.check(wgrad(dy.data_ptr(), x.data_ptr(), part.data_ptr(), dw.data_ptr(), b, c, n, h, w, s, dt, dwt, st),
                        "mrla_conv3x3_wgrad")
                torch.cuda.synchronize()
                key = f"{b}x{c}x{n}x{h}x{w}x{s} {dname} {wname}"
                entry = {}
                for name, t in (("part", part), ("dw", dw)):
                    assert not bool(torch.isnan(t).any()), (key, name)
                    raw = t.reshape(-1).view(torch.uint8).cpu()
                    entry[name] = {"elements": t.numel(), "sha256": hashlib.sha256(raw.numpy().tobytes()).hexdigest()}
                    torch.save(t.reshape(-1)[:KEEP].cpu(), os.path.join(out_dir, f"{len(index)}_{name}.pt"))
                index[key] = entry
                del part, dw
        del x32, dy32
        torch.cuda.empty_cache()
    with open(os.path.join(out_dir, "index.json"), "w") as f:
        json.dump({"library": L.LIB_PATH, "cases": index}, f, indent=1)
    print(f"{len(index)} cases from {L.LIB_PATH} -> {out_dir}")


def compare(dir_a, dir_b):
    import torch
    a, b = (json.load(open(os.path.join(d, "index.json"))) for d in (dir_a, dir_b))
    print(f"A = {a['library']}\nB = {b['library']}")
    assert list(a["cases"]) == list(b["cases"]) and a["library"] != b["library"]
    bad = 0
    for i, key in enumerate(a["cases"]):
        line = []
        for name in ("part", "dw"):
            ea, eb = a["cases"][key][name], b["cases"][key][name]
            assert ea["elements"] == eb["elements"]
            diff = 0
            if ea["sha256"] != eb["sha256"]:
                ta, tb = (torch.load(os.path.join(d, f"{i}_{name}.pt")) for d in (dir_a, dir_b))
                diff = max(1, int((ta.view(torch.uint8) != tb.view(torch.uint8)).view(ta.numel(), -1).any(1).sum()))
            bad += diff
            line.append(f"{name} {ea['elements']} elements, {diff} differ" + (" (of the first 2^20 kept)" if diff else ""))
        print(f"{key}: " + "; ".join(line))
    print(f"{len(a['cases'])} cases, {bad} differing elements")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
