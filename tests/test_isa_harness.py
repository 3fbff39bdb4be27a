"""The ISA audit's harness (tests/_isa.py) on a hand-written assembly text of two functions: no compiler, no GPU, milliseconds.
What the audit modules and tools/isa_diff.py rest on: the metadata and the counts belong to the right function, the loop
statistics count only what lies between the loop header and its back edge, and the fingerprint sees code, not comments."""
import _isa

ASM = """\
	.text
	.globl	_Z9with_loopPf
	.type	_Z9with_loopPf,@function
_Z9with_loopPf:                         ; @_Z9with_loopPf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_accvgpr_write_b32 a0, 0
	v_accvgpr_write_b32 a1, 0
	v_mfma_f32_32x32x2_f32 a[0:15], v0, v1, a[0:15]
	scratch_load_dword v9, off, off
	s_cbranch_scc1 .LBB0_3
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	v_mfma_f32_16x16x4_f32 a[0:3], v2, v3, a[0:3]
	v_mfma_f32_16x16x4_f32 a[0:3], v4, v5, a[0:3]
	v_accvgpr_mov_b32 a5, a4
	scratch_load_dword v10, off, off offset:4
	s_add_i32 s2, s2, -1
	s_cbranch_scc0 .LBB0_1
; %bb.2:
	v_mfma_f32_16x16x4_f32 a[0:3], v6, v7, a[0:3]
	v_accvgpr_read_b32 v8, a0
	s_cbranch_execz .LBB0_3
.LBB0_3:
	global_store_dword v0, v8, s[0:1]
	s_endpgm
.Lfunc_end0:
	.size	_Z9with_loopPf, .Lfunc_end0-_Z9with_loopPf
                                        ; -- End function
	.section	.AMDGPU.csdata,"",@progbits
; Kernel info:
; NumVgprs: 10
; NumAgprs: 16
; ScratchSize: 8
; Occupancy: 8
; LDSByteSize: 0 bytes/workgroup (compile time only)
	.text
	.globl	_Z7no_loopPf
	.type	_Z7no_loopPf,@function
_Z7no_loopPf:                           ; @_Z7no_loopPf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v1, 1.0                  ; v_mfma in a comment after code is no instruction at the line's start
	global_store_dword v0, v1, s[0:1]
	s_endpgm
.Lfunc_end1:
	.size	_Z7no_loopPf, .Lfunc_end1-_Z7no_loopPf
                                        ; -- End function
	.section	.AMDGPU.csdata,"",@progbits
; Kernel info:
; NumVgprs: 2
; NumAgprs: 0
; ScratchSize: 0
; Occupancy: 8
; LDSByteSize: 4096 bytes/workgroup (compile time only)
_ZL5table:
	.long	1
"""


def test_metadata_and_counts_belong_to_their_function():
    k = _isa.parse(ASM)
    assert sorted(k) == ["_Z7no_loopPf", "_Z9with_loopPf"]          # (_ZL5table: a label with no function end, no NumVgprs)
    loop, flat = k["_Z9with_loopPf"], k["_Z7no_loopPf"]
    assert [loop[m] for m in _isa.META] == [10, 16, 8, 8, 0] and [flat[m] for m in _isa.META] == [2, 0, 0, 8, 4096]
    assert loop["mfma"] == 4 and loop["mfma_16x16x4"] == 3 and flat["mfma"] == 0 and flat["mfma_16x16x4"] == 0
    assert (loop["accvgpr_write"], loop["accvgpr_read"], loop["accvgpr_mov"]) == (2, 1, 1)
    assert (flat["accvgpr_write"], flat["accvgpr_read"], flat["accvgpr_mov"]) == (0, 0, 0)
    assert _isa.family(k, "with_") == {"_Z9with_loopPf": loop}


def test_loop_statistics_stop_at_the_back_edge():
    loop = _isa.parse(ASM)["_Z9with_loopPf"]
    # before the header: 1 MFMA, 2 v_accvgpr_write, 1 scratch_; after the back edge: 1 MFMA, 1 v_accvgpr_read
    assert (loop["loop_mfma"], loop["loop_accvgpr"], loop["loop_scratch"]) == (2, 1, 1)


def test_no_loop_header_gives_none():
    flat = _isa.parse(ASM)["_Z7no_loopPf"]
    assert flat["loop_mfma"] is None and flat["loop_accvgpr"] is None and flat["loop_scratch"] is None


def test_fingerprint_sees_code_not_comments():
    base = _isa.fingerprint(ASM)
    assert sorted(base) == ["_Z7no_loopPf", "_Z9with_loopPf"] and base["_Z7no_loopPf"] != base["_Z9with_loopPf"]
    commented = ASM.replace("; =>This Inner Loop Header: Depth=1", "; =>another remark").replace("; %bb.2:", "; %bb.7:\n; a new comment line")
    assert commented != ASM and _isa.fingerprint(commented) == base
    # the function's ordinal in its local labels is its place in the file, not its code
    assert _isa.fingerprint(ASM.replace(".LBB0_", ".LBB5_").replace(".Lfunc_end0", ".Lfunc_end5")) == base
    edited = _isa.fingerprint(ASM.replace("s_add_i32 s2, s2, -1", "s_add_i32 s2, s2, -2"))
    assert edited["_Z9with_loopPf"] != base["_Z9with_loopPf"] and edited["_Z7no_loopPf"] == base["_Z7no_loopPf"]
