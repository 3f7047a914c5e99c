#!/usr/bin/env python3
"""Every answer the conv dispatch gives over a fixed grid of descriptors x epilogues, on the CPU (nothing is launched).

For each case: climsr_conv2d_fwd_kernel (and climsr_last_error when it names no kernel), climsr_conv2d_fwd_bn_parts,
climsr_conv2d_fwd_ch_parts with tiles_per_image; per descriptor and up in {1, 2}: climsr_conv2d_wgrad_kernel, _splits,
_workspace; per descriptor: climsr_conv_chunk_ex, _packed_k, _packed_rows.  The summary is a histogram of the kernel
names and refusals plus one SHA-256 per (in_c, out_c) block over the ordered text of every answer in the block.

tests/golden/conv_routes.json holds the summary of the library BEFORE a dispatch refactor (CLIMSR_HIP_LIB selects the
library, so build the parent commit elsewhere and point at it); tests/test_route_sweep.py recomputes it from the
library under test.  A route that moved changes a digest; to find it, write both tables and diff them:

    CLIMSR_HIP_LIB=/path/to/parent/libclimsr_hip.so python tools/route_sweep.py --table /tmp/parent.txt
    python tools/route_sweep.py --table /tmp/new.txt && diff /tmp/parent.txt /tmp/new.txt | head
    CLIMSR_HIP_LIB=/path/to/parent/libclimsr_hip.so python tools/route_sweep.py --write tests/golden/conv_routes.json
"""
import argparse
import ctypes
import hashlib
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IN_C = (4, 8, 32, 64, 80, 96, 112, 128, 256, 512)
OUT_C = (1, 16, 32, 48, 64, 80, 112, 128, 512)
KS = (1, 3, 5, 9)
STRIDE_UP = ((1, 1), (1, 2), (1, -2), (2, 1))
SIDE = (8, 16, 64, 256)
BATCH = (1, 32)
# (packed or wide channel strides (128, or 640 for more than 128 channels), input channel offset, output and residual
# channel offset)
LAYOUT = ((False, 0, 0), (True, 0, 0), (True, 8, 8), (True, 0, 4))
EPILOGUES = ("plain", "bias_lrelu", "bias_relu", "lrelu", "f32_out", "res1", "res1_res2", "f32_pull", "act3", "act4", "down2",
             "bn_part", "bn_part_z", "ch_part", "aux")
P = 0x1000  # a non-null operand: the queries never read through it


def epilogue(lib_mod, kind, ocs, oco):
    """(Epilogue, has_bias) of one of the fifteen kinds; residual / aux operands share the output's channel layout."""
    e = lib_mod.Epilogue(slope=0.2, alpha1=1.0, alpha2=1.0)
    bias = kind in ("bias_lrelu", "bias_relu", "res1", "res1_res2", "ch_part")

    def res1():
        e.res1, e.res1_cstride, e.res1_coff = P, ocs, oco

    if kind in ("bias_lrelu", "lrelu"):
        e.act = 1
    elif kind == "bias_relu":
        e.act = 2
    elif kind == "f32_out":
        e.out_mode = 1
    elif kind in ("res1", "res1_res2"):
        res1()
        e.alpha1 = 0.2
        if kind == "res1_res2":
            e.res2, e.res2_cstride, e.res2_coff, e.alpha2 = P, ocs, oco, 0.2
    elif kind == "f32_pull":
        res1()
        e.res_f32, e.out_mode = 1, 1
    elif kind in ("act3", "act4", "down2"):
        res1()
        e.act = 4 if kind == "act4" else 3
        e.down2 = int(kind == "down2")
    elif kind in ("bn_part", "bn_part_z"):
        e.bn_part = P
        if kind == "bn_part_z":
            e.bn_z, e.bn_z_cstride, e.bn_slope = P, ocs, 0.2
            e.bn_mean = e.bn_rstd = e.bn_gamma = e.bn_beta = P
    elif kind == "ch_part":
        e.ch_part = P
    elif kind == "aux":
        e.aux, e.aux_cstride, e.aux_coff, e.aux_scale = P, ocs, oco, 1.0
    return e, bias


def extras(lib_mod):
    """Refusals the grid's well-formed epilogues cannot reach: (ConvDesc, Epilogue or None, has_bias)."""
    def desc(side=64, out_side=None, **kw):
        d = lib_mod.ConvDesc(n=2, in_h=side, in_w=side, in_c=64, in_cstride=64, in_coff=0, up=1, ks=3, stride=1, pad=1,
                             out_h=out_side or side, out_w=out_side or side, out_c=64, out_cstride=64, out_coff=0, cc=64)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def ep(kind, **kw):
        e, _ = epilogue(lib_mod, kind, 64, 0)
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    return [
        (desc(), None, False),                               # null argument
        (desc(), ep("plain", act=5), False),                 # act out of range
        (desc(), ep("plain", act=3), False),                 # act 3 without res1
        (desc(), ep("aux", aux_coff=2), False),              # aux misaligned
        (desc(), ep("down2"), True),                         # down2 with a bias
        (desc(side=63, out_side=63), ep("down2"), False),    # down2 over an odd output
        (desc(in_c=128, in_cstride=128, out_c=128, out_cstride=128, cc=32), ep("bn_part_z", bn_mean=None), False),  # no statistics
        (desc(in_c=128, in_cstride=128, out_c=128, out_cstride=128, cc=32), ep("bn_part_z", bn_z_cstride=64), False),
        (desc(cc=0), ep("plain"), False),
        (desc(n=0), ep("plain"), False),
        (desc(up=3), ep("plain"), False),
        (desc(out_c=0), ep("plain"), False),                 # no outputs: the queries answer 0, nothing divides by it
        (desc(out_c=-3), ep("ch_part"), True),
        (desc(out_c=0, stride=2, out_side=32, in_c=64, cc=32), ep("bn_part"), False),
        # a stride-2 data gradient with BatchNorm-backward partials whose (unused) res1 stride fails dgrad_s2's size test
        (desc(n=32, side=128, out_side=256, up=-2, in_c=128, in_cstride=128, out_c=128, out_cstride=128, cc=32),
         ep("bn_part_z", bn_z_cstride=128, res1_cstride=1 << 20), False),
    ]


def sweep(table=None):
    from climsr_amd import _lib
    lib = _lib.load()
    tpi = ctypes.c_int32(0)
    names, refusals, blocks, kinds, eps = {}, {}, {}, {}, {}

    fwd_kernel, last_error = lib.climsr_conv2d_fwd_kernel, lib.climsr_last_error
    bn_parts, ch_parts, tpi_ref = lib.climsr_conv2d_fwd_bn_parts, lib.climsr_conv2d_fwd_ch_parts, ctypes.byref(tpi)

    def case(d, ep, bias):  # d, ep: ctypes.byref of the descriptor and the epilogue (or None)
        tpi.value = 0
        name = fwd_kernel(d, P if bias else None, ep).decode()
        if name:
            names[name] = names.get(name, 0) + 1
            err = ""
        else:
            err = last_error().decode()
            kind = kinds.get(err) or kinds.setdefault(err, re.sub(r"-?\d+", "#", err))
            refusals[kind] = refusals.get(kind, 0) + 1
        bn = bn_parts(d, ep)
        ch = ch_parts(d, ep, tpi_ref)
        return f"{name}|{err}|{bn}|{ch},{tpi.value}"

    for in_c in IN_C:
        for out_c in OUT_C:
            lines = []
            for ks in KS:
                for stride, up in STRIDE_UP:
                    cc = lib.climsr_conv_chunk_ex(in_c, ks, out_c, stride)
                    pk = f"cc={cc} k={lib.climsr_conv_packed_k(in_c, ks, cc)} rows={lib.climsr_conv_packed_rows(out_c)}"
                    for side in SIDE:
                        oh = side * 2 if up in (2, -2) else (side + stride - 1) // stride
                        for n in BATCH:
                            # (the offset layouts at the two middle sizes of the full batch only: they move alignment
                            # decisions, which no size or batch enters)
                            for wide, ico, oco in LAYOUT if n == 32 and side in (16, 64) else LAYOUT[:2]:
                                ics = (128 if in_c + ico <= 128 else 640) if wide else max(in_c, 8)
                                ocs = (128 if out_c + oco <= 128 else 640) if wide else max((out_c + 7) // 8 * 8, 8)
                                d = _lib.ConvDesc(n=n, in_h=side, in_w=side, in_c=in_c, in_cstride=ics, in_coff=ico, up=up, ks=ks,
                                                  stride=stride, pad=ks // 2, out_h=oh, out_w=oh, out_c=out_c, out_cstride=ocs,
                                                  out_coff=oco, cc=cc)
                                dref = ctypes.byref(d)
                                head = f"{in_c}>{out_c} k{ks} s{stride} u{up} {side}^2 n{n} cs{ics}+{ico}/{ocs}+{oco}"
                                lines.append(f"{head} {pk}")
                                if up != -2:  # (weight gradients: up 1 / 2 only)
                                    wn = lib.climsr_conv2d_wgrad_kernel(dref).decode()
                                    if wn:
                                        names[wn] = names.get(wn, 0) + 1
                                    ns = lib.climsr_conv2d_wgrad_splits(dref)
                                    lines.append(f"{head} wgrad {wn}|{ns}|{lib.climsr_conv2d_wgrad_workspace(dref, ns)}")
                                for kind in EPILOGUES:
                                    key = (kind, ocs, oco)
                                    if key not in eps:
                                        e, bias = epilogue(_lib, kind, ocs, oco)
                                        eps[key] = (e, ctypes.byref(e), bias)
                                    lines.append(f"{head} {kind} {case(dref, eps[key][1], eps[key][2])}")
            blocks[f"{in_c}>{out_c}"] = lines
    blocks["extras"] = [f"extra{i} {case(ctypes.byref(d), ctypes.byref(e) if e is not None else None, bias)}"
                        for i, (d, e, bias) in enumerate(extras(_lib))]
    if table:
        with open(table, "w") as f:
            for lines in blocks.values():
                f.write("\n".join(lines) + "\n")
    return {"cases": sum(names[k] for k in names if "wgrad" not in k) + sum(refusals.values()),
            "names": dict(sorted(names.items())), "refusals": dict(sorted(refusals.items())),
            "blocks": {k: hashlib.sha256("\n".join(v).encode()).hexdigest() for k, v in blocks.items()}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", metavar="JSON", help="write the summary (the fixture; from the PARENT library only)")
    ap.add_argument("--table", metavar="TXT", help="also write every answer as text (to diff two libraries)")
    args = ap.parse_args()
    got = sweep(args.table)
    fwd = [n for n in got["names"] if "wgrad" not in n]
    print(f"{got['cases']} forward cases; {sum(got['names'].values())} named answers, {len(fwd)} forward and {len(got['names']) - len(fwd)} weight-gradient "
          f"kernel names, {sum(got['refusals'].values())} refusals of {len(got['refusals'])} kinds")
    if args.write:
        with open(args.write, "w") as f:
            json.dump(got, f, indent=0, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
