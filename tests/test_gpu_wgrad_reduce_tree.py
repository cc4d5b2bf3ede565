"""The summation tree of the weight gradient's slab sum (csrc/cy_wgrad.hip wgrad_reduce_block), checked against the tree
itself rather than against another launch: cy_wgrad_reduce_batched on hand-made random f32 slabs, the expected value
built on the CPU with explicit sequential f32 tensor adds --

    group g:   acc_g = ((0 + slab[g]) + slab[g + SG]) + ...        (increasing slab index)
    output:    ((acc_0 + acc_1) + acc_2) + ... + acc_{SG-1}         (group order)
    dW:        old + output when the entry accumulates, else output

-- and torch.equal.  IEEE f32 addition is the same on both sides, so any reordering inside the kernel shows as a
mismatch.  The first layer's partial sum (64 slices, then the slices in order) is restated the same way for one mixed
table.  The table is laid out as in tests/test_gpu_wgrad_batched.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (S, SG, Cout, Cin, co_pad, ci_pad)
CONV_CASES = [
    (1, 1, 32, 32, 32, 32),
    (3, 1, 32, 32, 32, 32),
    (8, 4, 32, 32, 32, 32),
    (256, 32, 32, 32, 32, 32),
    (4, 1, 64, 128, 96, 192),  # padded slabs: co_pad / ci_pad larger than Cout / Cin
]


def _conv_entry(S, SG, Cout, Cin, co_pad, ci_pad, accumulate, g):
    """(entry, expected dW, tensors to keep alive)"""
    from cyhip import _lib
    ws = torch.randn(S, 9, co_pad, ci_pad, generator=g)
    base = torch.randn(Cout, Cin, 3, 3, generator=g)
    groups = []
    for grp in range(SG):
        acc = torch.zeros(9, co_pad, ci_pad)
        for q in range(grp, S, SG):
            acc = acc + ws[q]
        groups.append(acc)
    total = groups[0]
    for grp in range(1, SG):
        total = total + groups[grp]
    out = total[:, :Cout, :Cin].permute(1, 2, 0).reshape(Cout, Cin, 3, 3).contiguous()  # [tap][co][ci] -> [co][ci][tap]
    want = base + out if accumulate else out
    ws_d = ws.to(DEV)
    dw_d = base.to(DEV) if accumulate else torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
    e = _lib.WgradReduceEntry()
    e.ws, e.dw, e.kind = ws_d.data_ptr(), dw_d.data_ptr(), 0
    e.S, e.SG, e.Cout, e.Cin, e.co_pad, e.ci_pad, e.accumulate = S, SG, Cout, Cin, co_pad, ci_pad, accumulate
    opb = 256 // SG
    e.blocks = (Cout * (Cin // 4) + opb - 1) // opb
    return e, want, (ws_d, dw_d)


def _first_entry(nblk, Cout, Cin, accumulate, g):
    from cyhip import _lib
    total = Cout * Cin * 9
    ws = torch.randn(nblk, total, generator=g)
    base = torch.randn(Cout, Cin, 3, 3, generator=g)
    slices = []
    for sl in range(64):
        acc = torch.zeros(total)
        for q in range(sl, nblk, 64):
            acc = acc + ws[q]
        slices.append(acc)
    t = torch.zeros(total)
    for sl in range(64):
        t = t + slices[sl]
    out = t.reshape(Cout, Cin, 3, 3)
    want = base + out if accumulate else out
    ws_d = ws.to(DEV)
    dw_d = base.to(DEV) if accumulate else torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
    e = _lib.WgradReduceEntry()
    e.ws, e.dw, e.kind = ws_d.data_ptr(), dw_d.data_ptr(), 1
    e.S, e.SG, e.Cout, e.Cin, e.accumulate = nblk, 64, Cout, Cin, accumulate
    e.blocks = (total + 3) // 4
    return e, want, (ws_d, dw_d)


def _batched(entries):
    from cyhip import _lib, ops
    arr = (_lib.WgradReduceEntry * len(entries))(*entries)
    _lib.call("cy_wgrad_reduce_batched", arr, len(entries), ops._stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "S{}-SG{}-{}x{}".format(*c[:4]))
def test_slab_sum_is_the_stated_tree(case, accumulate):
    g = torch.Generator().manual_seed(17 + accumulate)
    e, want, keep = _conv_entry(*case, accumulate, g)
    _batched([e])
    got = keep[1].cpu()
    assert torch.equal(got, want), (case, accumulate, (got - want).abs().max().item())


def test_mixed_table_with_a_first_layer_entry():
    g = torch.Generator().manual_seed(23)
    made = [_conv_entry(8, 4, 32, 32, 32, 32, 1, g), _first_entry(100, 32, 1, 1, g),
            _conv_entry(4, 1, 64, 128, 96, 192, 0, g), _first_entry(7, 32, 1, 0, g),
            _conv_entry(256, 32, 32, 32, 32, 32, 1, g)]
    _batched([m[0] for m in made])
    for i, (_, want, keep) in enumerate(made):
        got = keep[1].cpu()
        assert torch.equal(got, want), (i, (got - want).abs().max().item())
