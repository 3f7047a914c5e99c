"""tools/isa_counts.py on a hand-written assembly fragment: the instruction classes it counts per kernel, the scratch
size it takes from the kernel descriptor, and the Makefile flags it compiles with (no compiler, no GPU needed)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("isa_counts", os.path.join(ROOT, "tools", "isa_counts.py"))
isa_counts = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa_counts)

ASM = """
	.text
_Z6helperv:
	s_mov_b32 s0, 1
_Z1kv:                                  ; @_Z1kv
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	s_waitcnt lgkmcnt(0)
	s_cmp_eq_u32 s0, 1
	s_cbranch_scc1 .LBB0_2
	v_mov_b32_e32 v0, 0                     ; a comment with v_add_f32 in it
	;;#ASMSTART
	v_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]
	;;#ASMEND
.LBB0_2:
	v_add_f32_e32 v1, v0, v0
	s_add_u32 s2, s0, s1
	s_nop 0
	s_branch .LBB0_3
.LBB0_3:
	buffer_store_dword v1, v0, s[8:11], 0 offen
	s_endpgm
.Lfunc_end0:
	v_mov_b32_e32 v9, 0
	.amdhsa_kernel _Z1kv
		.amdhsa_private_segment_fixed_size 16
	.end_amdhsa_kernel
"""


def test_counts_per_kernel():
    res = isa_counts.count(ASM)
    assert list(res) == ["_Z1kv"], "only .amdhsa_kernel symbols, and nothing past .Lfunc_end"
    assert res["_Z1kv"] == dict(branch=2, salu=2, valu=2, mfma=1, scratch=16)


def test_flags_follow_the_makefile():
    _hipcc, flags = isa_counts.make_flags("data.hip")
    assert "-O3" in flags and any(f.startswith("--offload-arch=gfx") for f in flags)
    assert "-ffp-contract=off" in flags, "data.o's own CXXFLAGS += line"
    assert "-ffp-contract=off" not in isa_counts.make_flags("conv_wr.hip")[1]
