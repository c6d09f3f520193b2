"""What tests/test_gpu_gemm_memory.py, tests/test_gpu_attention_memory.py and tests/test_gpu_lora_memory.py share: a Placer that puts every
pointer of one raw call into an arena of tests/arena.py, and the contract those modules assert on it (their docstrings number it 1 - 7).

A module gives  launch(P) -> rc  -- it places its operands with P.inp / P.out / P.ws, fills the C struct with their addresses and calls the
entry point through unirec_amd._lib --, wrapper() -> {output name: tensor} from the hip.* wrapper on ordinary tensors, and
reference(outs), the reference check of the entry point's own float64 module."""
import torch

from tests import arena
from unirec_amd import _lib

DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32, "u8": torch.uint8, "i32": torch.int32}


def raw_bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw_bytes(a), raw_bytes(b))


class Placer:
    """the arenas of one raw call.  interior: what the workspace holds; out_fill: what every output element holds before the call (the pads
    and guards of an output always hold arena.OUT); short: bytes the sized workspace is cut by."""

    def __init__(self, interior=arena.NAN, out_fill=arena.OUT, short=0):
        self.interior, self.out_fill, self.short = interior, out_fill, short
        self.arenas, self.inputs, self.outputs, self.unwritten, self.workspaces = {}, {}, {}, set(), []
        self.rc, self.error = None, ""

    def inp(self, name, t, align=16, ld=None):
        """a dense tensor of any shape, or (ld given) a 2-D tensor with row stride ld"""
        t = t.to(DEV)
        fill = arena.NAN if t.is_floating_point() else arena.OUT
        if ld is None:
            whole, view = arena.place(t, align, fill)
        else:
            whole, view = arena.place(t, align, fill, ld=ld, guard=arena.guard_for(ld, t.element_size()))
        self.arenas[name], self.inputs[name] = (whole, view), t.clone()
        return view

    def out(self, name, shape, dtype, align=16, ld=None, written=True):
        interior = None if self.out_fill == arena.OUT else self.out_fill
        esize = torch.empty((), dtype=dtype).element_size()
        if ld is None:
            n = 1
            for s in shape:
                n *= int(s)
            whole, raw = arena.place(n * esize, align, arena.OUT, device=DEV, interior=interior)
            view = arena.typed(raw, dtype, tuple(shape))
            self.arenas[name] = (whole, raw)
        else:
            whole, view = arena.place((int(shape[0]), int(shape[1]), dtype), align, arena.OUT, device=DEV, interior=interior, ld=ld,
                                      guard=arena.guard_for(ld, esize))
            self.arenas[name] = (whole, view)
        self.outputs[name] = view
        if not written:
            self.unwritten.add(name)
        return view

    def ws(self, name, nbytes, align=16):
        """a sized workspace of exactly nbytes (less `short`), its interior the poison of this run"""
        whole, view = arena.place(int(nbytes) - self.short, align, arena.OUT, device=DEV, interior=self.interior)
        self.arenas[name] = (whole, view)
        self.workspaces.append(name)
        return view

    def finish(self, rc):
        torch.cuda.synchronize()
        self.rc = int(rc)
        self.error = _lib.load().ur_last_error().decode("utf-8", "replace") if self.rc != 0 else ""
        return self


def check_placement(P, what):
    """assertions 2 and 3 on one finished run"""
    for name, (whole, view) in P.arenas.items():                                                               # 2
        assert arena.intact(whole, view), f"{what}: a guard of {name} was written"
        assert arena.pads_intact(whole), f"{what}: a pad column of {name} was written"
    for name, t in P.inputs.items():
        assert same_bits(P.arenas[name][1], t), f"{what}: input {name} was written"
    for name, view in P.outputs.items():                                                                       # 3
        if name in P.unwritten:
            assert bool((raw_bytes(view) == P.out_fill).all()), f"{what}: {name} was written, the header says it is not"
        elif P.out_fill == arena.OUT:
            assert arena.all_written(view), f"{what}: {name} keeps elements nobody stored"


def refused_untouched(P, what, word="workspace"):
    """assertion 7 on one finished run"""
    assert P.rc < 0 and word in P.error, (what, P.rc, P.error)
    for name, (whole, view) in P.arenas.items():
        if name in P.outputs or name in P.workspaces:
            assert arena.untouched(whole), f"{what}: a refused call wrote {name}"
        else:
            assert arena.intact(whole, view) and arena.pads_intact(whole), name
    for name, t in P.inputs.items():
        assert same_bits(P.arenas[name][1], t), f"{what}: a refused call wrote input {name}"


def memory_contract(what, launch, wrapper, reference, sized=False, poisons=True):
    """assertions 1 - 7.  sized: the call takes a sized workspace (7 applies).  poisons: the call has a workspace of either kind, so the
    0x00 interior is run too.  Returns the outputs of the first run."""
    plan = [(arena.NAN, arena.OUT)] + ([(arena.ZERO, arena.OUT)] if poisons else []) + [(arena.NAN, arena.NAN)]
    runs = []
    for interior, out_fill in plan:
        P = Placer(interior, out_fill)
        P.finish(launch(P))
        assert P.rc == 0, (what, P.rc, P.error)                                                                # 1
        check_placement(P, what)                                                                               # 2, 3
        runs.append(P)
    live = [n for n in runs[0].outputs if n not in runs[0].unwritten]
    outs = {n: runs[0].outputs[n].clone() for n in live}
    for P, (interior, out_fill) in zip(runs[1:], plan[1:]):                                                    # 6
        for n in live:
            assert same_bits(P.outputs[n], outs[n]), (f"{what}: {n} depends on what the " +
                                                      ("outputs held before the call" if out_fill != arena.OUT else "workspace held"))
    want = wrapper()                                                                                           # 4
    assert want and set(want) <= set(outs), f"{what}: the wrapper's outputs {sorted(want)} are outputs of the raw call {sorted(outs)}"
    for n, t in want.items():
        if t.element_size() == 2:      # (what all_written asks of a 16-bit output: no legitimate result reads as the fill)
            assert not bool((t.contiguous().view(torch.int16) == arena.OUT_HALF).any()), f"{what}: {n} legitimately holds 0x5A5A; choose other inputs"
        assert same_bits(t, outs[n]), f"{what}: {n} differs from the wrapper's"
    reference(outs)                                                                                            # 5
    if sized:                                                                                                  # 7
        P = Placer(arena.OUT, arena.OUT, short=1)
        refused_untouched(P.finish(launch(P)), what)
    return outs
