"""GPU, kernel level, through the C ABI: mrla_conv3x3_weight_bank_refresh (mrla_amd/csrc/weight_bank.hip).

One launch over a table of four fp32 weights [n, c, 3, 3] of different sizes -- (n, c) = (64, 64), (128, 64), (64, 128),
(192, 128): the last has tile counts that are no power of two, and the workgroups of the smaller entries past their own
tiles return -- two of them contiguous and two channels_last, in bf16 and fp16:
  * w16 is torch.equal to w.to(dt) in channels_last, wflip to w.to(dt).flip(2, 3).transpose(0, 1) in channels_last;
  * a NaN-filled guard of 64 elements on both sides of every destination is untouched;
  * +-inf, NaN, values that overflow fp16, values that round up into the next binade, subnormals and signed zeros come out as
    a torch cast gives them;
  * a captured refresh, replayed three times with the masters changed in between, follows the masters each time."""
import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last
SIZES = ((64, 64), (128, 64), (64, 128), (192, 128))        # (n, c)
GUARD = 64
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _masters(seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ws = []
    for i, (n, c) in enumerate(SIZES):
        w = torch.randn((n, c, 3, 3), device="cuda", generator=g) * (0.05 if i % 2 else 3.0)
        ws.append(w.contiguous(memory_format=CL) if i in (1, 3) else w.contiguous())
    assert [w.is_contiguous() for w in ws] == [True, False, True, False]
    return ws


class _Bank:
    """Guarded destinations and the device table of `ws`."""

    def __init__(self, ws, dt):
        self.ws, self.dt, self.bufs, rows = ws, dt, [], []
        for w in ws:
            n, c = w.shape[:2]
            numel = n * c * 9
            pair = []
            for _ in range(2):
                buf = torch.full((numel + 2 * GUARD,), float("nan"), dtype=dt, device="cuda")
                assert buf[GUARD:].data_ptr() % 8 == 0
                pair.append(buf)
            self.bufs.append(pair)
            rows.append([w.data_ptr(), pair[0][GUARD:].data_ptr(), pair[1][GUARD:].data_ptr(), (n << 32) | c,
                         0 if w.is_contiguous() else 1])
        self.table = torch.tensor(rows, dtype=torch.int64).cuda()
        self.max_tiles = max(9 * (w.shape[0] // 64) * (w.shape[1] // 64) for w in ws)

    def refresh(self):
        from mrla_amd import _lib as L
        code = L.BF16 if self.dt == torch.bfloat16 else L.F16
        L.call("mrla_conv3x3_weight_bank_refresh", self.table.data_ptr(), len(self.ws), self.max_tiles, code,
               torch.cuda.current_stream().cuda_stream)

    def copies(self, i):
        """(w16 as a channels_last [n, c, 3, 3], wflip as a channels_last [c, n, 3, 3]) of entry i."""
        n, c = self.ws[i].shape[:2]
        w16 = self.bufs[i][0][GUARD:-GUARD].view(n, 3, 3, c).permute(0, 3, 1, 2)
        wflip = self.bufs[i][1][GUARD:-GUARD].view(c, 3, 3, n).permute(0, 3, 1, 2)
        return w16, wflip

    def check(self):
        torch.cuda.synchronize()
        for i, w in enumerate(self.ws):
            w16, wflip = self.copies(i)
            want = w.detach().to(self.dt)
            want16 = want.contiguous(memory_format=CL)
            wantflip = want.flip(2, 3).transpose(0, 1).contiguous(memory_format=CL)
            assert w16.is_contiguous(memory_format=CL) and wflip.is_contiguous(memory_format=CL)
            for name, got, exp in (("w16", w16, want16), ("wflip", wflip, wantflip)):
                # NaN exactly where the cast gives NaN (a NaN's payload is nobody's contract); every other element bit for
                # bit, the sign of a zero included
                nan = torch.isnan(exp)
                assert torch.equal(torch.isnan(got), nan), (i, name)
                assert torch.equal(got.contiguous().view(torch.int16).masked_fill(nan, 0),
                                   exp.contiguous().view(torch.int16).masked_fill(nan, 0)), (i, name)
                if not bool(nan.any()):
                    assert torch.equal(got, exp), (i, name)
            for buf in self.bufs[i]:
                assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), (i, "guard")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_one_launch_casts_and_flips_four_weights_of_different_sizes(dt):
    bank = _Bank(_masters(), DTYPES[dt])
    bank.refresh()
    bank.check()
    # the flip is the one the input gradient needs: wflip[c, n, kh, kw] = w16[n, c, 2 - kh, 2 - kw]
    w16, wflip = bank.copies(3)
    assert torch.equal(wflip[5, 7, 0, 2], w16[7, 5, 2, 0]) and torch.equal(wflip[100, 191, 1, 0], w16[191, 100, 1, 2])


@pytest.mark.parametrize("dt", list(DTYPES))
def test_special_values_come_out_as_a_torch_cast_gives_them(dt):
    ws = _masters(1)
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), 65504.0, 65520.0, 65519.99, -65520.0, 7e4, -1e30,
                            3.4028235e38, -3.4028235e38, 3.3895314e38, 1e-41, -1e-41, 6e-8, 2.9e-8, 0.0, -0.0,
                            1.00390625, 1.01171875, 1.99609375, 0.99999994, 5.9604645e-08, 1.1754944e-38],
                           device="cuda")
    with torch.no_grad():
        for w in ws:
            flat = w.view(-1) if w.is_contiguous() else w.permute(0, 2, 3, 1).reshape(-1)       # (views of the storage)
            assert flat.data_ptr() == w.data_ptr()
            idx = torch.arange(0, flat.numel(), flat.numel() // 997, device="cuda")[:special.numel() * 40]
            flat[idx] = special.repeat(40)[:idx.numel()]
        assert all(bool(torch.isinf(w).any()) and bool(torch.isnan(w).any()) for w in ws)
    bank = _Bank(ws, DTYPES[dt])
    bank.refresh()
    bank.check()
    if dt == "fp16":                       # overflow to +-inf happened, as in torch
        assert bool(torch.isinf(bank.copies(0)[0]).sum() > torch.isinf(ws[0]).sum())


@pytest.mark.parametrize("dt", list(DTYPES))
def test_a_captured_refresh_follows_the_masters_on_every_replay(dt):
    ws = _masters(2)
    bank = _Bank(ws, DTYPES[dt])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bank.refresh()                                           # warm-up on a side stream, as a capture wants it
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bank.refresh()
    for step in range(3):
        with torch.no_grad():
            for i, w in enumerate(ws):
                w.mul_(-0.5 - step).add_(0.01 * (i + 1))
        for pair in bank.bufs:                                   # poison what the previous replay wrote
            for buf in pair:
                buf[GUARD:-GUARD].fill_(float("nan"))
        graph.replay()
        bank.check()
