"""tools/isa_diff.py on hand-written assembly fragments: kernel bodies that are the same up to block-label numbers and
comments, a one-instruction difference, a symbol on one side only and a symbol defined twice (no compiler, no GPU)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa_diff)


def kernel(name, fn, add="v_add_f32_e32 v1, v0, v0", note=""):
    """One kernel as function number `fn` of its unit (the number its block labels and .Lfunc_end carry)."""
    return f"""
	.globl	{name}
	.p2align	8
	.type	{name},@function
{name}:                                  ; @{name} {note}
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	s_cbranch_scc1 .LBB{fn}_2
	v_mov_b32_e32 v0, 0                     ; {note}
.LBB{fn}_2:
	{add}
	s_cbranch_scc0 .LBB{fn}_4
	s_branch .LBB{fn}_2
.LBB{fn}_4:
	s_endpgm
.Lfunc_end{fn}:
	.size	{name}, .Lfunc_end{fn}-{name}
	.amdhsa_kernel {name}
		.amdhsa_private_segment_fixed_size 0
	.end_amdhsa_kernel
"""


HELPER = "_Z6helperv:\n\ts_mov_b32 s0, 1\n\ts_setpc_b64 s[30:31]\n.Lfunc_end9:\n"


def run(old, new):
    lines, ok = isa_diff.compare(isa_diff.bodies(old), isa_diff.bodies(new))
    return lines, ok


def test_same_after_label_renumbering_and_comment_stripping():
    old = kernel("_Z1av", 0) + kernel("_Z1bv", 1)
    new = HELPER + kernel("_Z1bv", 7, note="moved, v_sub_f32 in a comment") + kernel("_Z1av", 3)
    lines, ok = run(old, new)
    assert ok, lines
    assert [ln.split()[0] for ln in lines[:-1]] == ["SAME", "SAME"]
    assert lines[-1].startswith("2 old symbols, 2 new: 2 same, 0 differ")
    body = isa_diff.bodies(old)["_Z1av"][0]
    assert len(body) == 9, "7 instructions and 2 block labels, no directives, no comments"


def test_one_instruction_differs():
    old = kernel("_Z1av", 0) + kernel("_Z1bv", 1)
    new = kernel("_Z1av", 0) + kernel("_Z1bv", 1, add="v_add_f32_e32 v1, v0, v1")
    lines, ok = run(old, new)
    assert not ok
    assert [ln.split()[0] for ln in lines[:-1]] == ["SAME", "DIFF"] and "b" in lines[1]
    assert lines[1].split()[1:3] == ["9", "9"], "both lengths"
    assert "1 same, 1 differ" in lines[-1]


def test_branch_to_another_block_differs():
    """Renumbering must keep WHICH block a branch names."""
    new = kernel("_Z1av", 0).replace("s_branch .LBB0_2", "s_branch .LBB0_4")
    assert not run(kernel("_Z1av", 0), new)[1]


def test_symbol_missing_on_one_side():
    both = kernel("_Z1av", 0)
    lines, ok = run(both + kernel("_Z1bv", 1), both)
    assert not ok and any(ln.startswith("ONLY old") and "b" in ln for ln in lines)
    lines, ok = run(both, both + kernel("_Z1cv", 1))
    assert not ok and any(ln.startswith("ONLY new") and "c" in ln for ln in lines)
    assert "1 on one side only" in lines[-1]


def test_symbol_defined_twice():
    one = kernel("_Z1av", 0)
    lines, ok = run(one, one + kernel("_Z1av", 5))  # (two units of the new side that both instantiate it)
    assert not ok and any(ln.startswith("TWICE new x2") for ln in lines)
    assert "1 defined more than once" in lines[-1]
