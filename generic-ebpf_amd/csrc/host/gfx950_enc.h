// gfx950_enc.h — the gfx950 machine-word encoder of the host compiler (asm_cc*.cpp, asm_jit.cpp).
//
// Encodings: VOP1/VOP2/VOPC (e32, literal allowed in src0), VOP3 (no literal on gfx9), SOP1, SOP2,
// SOPC, SOPP, DS, global loads.  Field layouts and opcodes are from llvm-mc -show-encoding for
// gfx950; tests/test_compile.py checks decoded forms.  No assembler stands between this encoder
// and the hardware: every instruction word either file emits is spelled here, by name.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "asm_handlers.h"

// source operand codes (SGPR n = n, inline constant v in 0..64 = 128 + v)
enum : uint32_t {
	SRC_VCC = 106, SRC_EXEC = 126, SRC_LIT = 255, VGPR0 = 256,
};
// VOP2 opcodes (bits 30:25)
enum : uint32_t {
	V2_CNDMASK_B32 = 0x00, V2_LSHRREV_B32 = 0x10, V2_LSHLREV_B32 = 0x12, V2_AND = 0x13, V2_OR = 0x14,
	V2_XOR = 0x15, V2_ADD_U32 = 0x34, V2_SUB_U32 = 0x35, V2_SUBREV_U32 = 0x36, V2_SUB_CO_U32 = 0x1a,
	V2_SUBB_CO_U32 = 0x1d,
};
// VOP1 opcodes (bits 16:9)
enum : uint32_t { V1_MOV_B32 = 0x01, V1_READFIRSTLANE_B32 = 0x02, V1_MOV_B64 = 0x38 };
// VOP3 opcodes (bits 25:16)
enum : uint32_t {
	V3_MAD_U32_U24 = 0x1c3, V3_BFE_U32 = 0x1c8, V3_ALIGNBYTE = 0x1cf, V3_MAD_U64_U32 = 0x1e8,
	V3_PERM_B32 = 0x1ed, V3_ADD3_U32 = 0x1ff, V3_LSHL_ADD_U64 = 0x208, V3_MUL_LO_U32 = 0x285,
	V3_LSHLREV_B64 = 0x28f, V3_LSHRREV_B64 = 0x290, V3_LSHL_ADD_U32 = 0x1fd,
};
// DS opcodes (bits 24:17)
enum : uint32_t {
	DS_ADD_U32 = 0x00, DS_WRITE_B32 = 0x0d, DS_WRITE2_B32 = 0x0e, DS_WRITE_B8 = 0x1e,
	DS_WRITE_B16 = 0x1f, DS_READ_B32 = 0x36, DS_READ2_B32 = 0x37, DS_READ_U8 = 0x3a,
	DS_READ_U16 = 0x3c,
};
// VOPC compare codes: base + {lt 1, eq 2, le 3, gt 4, ne 5, ge 6}
enum : uint32_t { VC_I32 = 0xc0, VC_U32 = 0xc8, VC_I64 = 0xe0, VC_U64 = 0xe8 };
enum { P_LT = 1, P_EQ = 2, P_LE = 3, P_GT = 4, P_NE = 5, P_GE = 6 };
// SOP1 opcodes (bits 15:8)
enum : uint32_t {
	S1_MOV_B32 = 0x00, S1_MOV_B64 = 0x01, S1_BCNT1_I32_B64 = 0x0d, S1_SETPC_B64 = 0x1d,
	S1_SWAPPC_B64 = 0x1e, S1_AND_SAVEEXEC_B64 = 0x20,
};
// SOP2 opcodes (bits 29:23)
enum : uint32_t {
	S2_ADD_U32 = 0x00, S2_ADDC_U32 = 0x04, S2_AND_B64 = 0x0d, S2_OR_B32 = 0x0e, S2_ANDN2_B64 = 0x13,
	S2_LSHR_B32 = 0x1e,
};
// SOPC opcodes (bits 22:16)
enum : uint32_t {
	SC_CMP_LG_U32 = 0x07, SC_CMP_GT_U32 = 0x08, SC_BITCMP1_B32 = 0x0d, SC_SET_GPR_IDX_ON = 0x11,
};
// SOPP opcodes (bits 22:16)
enum : uint32_t {
	SP_BRANCH = 0x02, SP_CBRANCH_SCC0 = 0x04, SP_CBRANCH_SCC1 = 0x05, SP_CBRANCH_EXECZ = 0x08,
	SP_CBRANCH_EXECNZ = 0x09, SP_WAITCNT = 0x0c, SP_SET_GPR_IDX_OFF = 0x1c,
};
// global_load_{ubyte, ushort, dword, dwordx2} (bits 24:18), by log2 of the access size
const uint32_t GLOBAL_LOAD[4] = {0x10, 0x12, 0x14, 0x15};

struct opnd {
	uint32_t code;
	uint32_t lit = 0;
};

inline bool
inline_i64(int64_t v, uint32_t *code)
{
	if (v >= 0 && v <= 64) {
		*code = 128 + (uint32_t)v;
		return true;
	}
	if (v >= -16 && v <= -1) {
		*code = 192 + (uint32_t)(-v);
		return true;
	}
	return false;
}

inline opnd
vreg(int n)
{
	return opnd{VGPR0 + (uint32_t)n};
}

inline opnd
sreg(int n)
{
	return opnd{(uint32_t)n};
}

// 32-bit constant for an e32 src0 / SOP source: inline constant or literal
inline opnd
k32(uint32_t v)
{
	uint32_t c;
	if (inline_i64((int64_t)(int32_t)v, &c))
		return opnd{c};
	return opnd{SRC_LIT, v};
}

// gfx9 (gfx950 included) VOP3 reads at most one SGPR (or VCC / EXEC / M0) through the constant
// bus; a second one reads garbage and no assembler stands between this encoder and the hardware.
// Every VOP3 the compiler emits is checked (cc_bus_violations, asm_jit_emit fails the build).
inline thread_local unsigned g_bus_violations = 0;

inline bool
is_sgpr_src(uint32_t c)
{
	return c <= 127 || (c >= 251 && c <= 253);
}

struct enc {
	std::vector<uint8_t> &b;
	void w(uint32_t x)
	{
		for (int i = 0; i < 4; i++)
			b.push_back((uint8_t)(x >> (8 * i)));
	}
	void lit(const opnd &s)
	{
		if (s.code == SRC_LIT)
			w(s.lit);
	}
	void vop2(uint32_t op, int vdst, opnd s0, int vsrc1)
	{
		w((op << 25) | ((uint32_t)vdst << 17) | ((uint32_t)vsrc1 << 9) | s0.code);
		lit(s0);
	}
	void vop1(uint32_t op, int vdst, opnd s0)
	{
		w((0x3fu << 25) | ((uint32_t)vdst << 17) | (op << 9) | s0.code);
		lit(s0);
	}
	void vopc(uint32_t op, opnd s0, int vsrc1)
	{
		w((0x3eu << 25) | (op << 17) | ((uint32_t)vsrc1 << 9) | s0.code);
		lit(s0);
	}
	// VOP3 (a and b forms); sources are 9-bit codes, never a literal on gfx9
	void vop3(uint32_t op, int vdst, uint32_t s0, uint32_t s1, uint32_t s2, int sdst = 0)
	{
		const uint32_t src[3] = {s0, s1, s2};
		// (two-source encodings: the compares, v_mul_lo_u32, the 64-bit shifts ignore src2)
		const int nsrc = (op < 0x100 || op == V3_MUL_LO_U32 || op == V3_LSHLREV_B64 ||
				  op == V3_LSHRREV_B64) ? 2 : 3;
		uint32_t bus = UINT32_MAX;
		for (int i = 0; i < nsrc; i++) {
			const uint32_t x = src[i];
			if (!is_sgpr_src(x) || x == bus)
				continue;
			if (bus != UINT32_MAX) {
				g_bus_violations++;
				if (getenv("EBPF_CC_BUS_DEBUG"))
					fprintf(stderr, "VOP3 op %#x reads SGPRs %u and %u\n", op, bus, x);
			}
			bus = x;
		}
		w((0x34u << 26) | (op << 16) | ((uint32_t)sdst << 8) | (uint32_t)vdst);
		w(s0 | (s1 << 9) | (s2 << 18));
	}
	void ds(uint32_t op, int addr, int data0, int data1, int vdst, uint32_t off0, uint32_t off1 = 0)
	{
		w((0x36u << 26) | (op << 17) | (off1 << 8) | off0);
		w((uint32_t)addr | ((uint32_t)data0 << 8) | ((uint32_t)data1 << 16) | ((uint32_t)vdst << 24));
	}
	// global_load of 1 << zi bytes: vdst = [v[vaddr:vaddr+1] + off] (no SGPR base, off < 4096)
	void global_load(int zi, int vdst, int vaddr, uint32_t off)
	{
		w(0xdc008000u | (GLOBAL_LOAD[zi] << 18) | off);
		w((uint32_t)vaddr | (0x7fu << 16) | ((uint32_t)vdst << 24));
	}
	void sop1(uint32_t op, int sdst, opnd s0)
	{
		w(0xbe800000u | ((uint32_t)sdst << 16) | (op << 8) | s0.code);
		lit(s0);
	}
	void sop2(uint32_t op, int sdst, opnd s0, opnd s1)
	{
		w(0x80000000u | (op << 23) | ((uint32_t)sdst << 16) | (s1.code << 8) | s0.code);
		lit(s0);
		lit(s1);
	}
	void sopc(uint32_t op, uint32_t s0, uint32_t s1) { w(0xbf000000u | (op << 16) | (s1 << 8) | s0); }
	void sopp(uint32_t op, uint32_t simm16 = 0) { w(0xbf800000u | (op << 16) | (simm16 & 0xffffu)); }
	// s_waitcnt vmcnt(vm) lgkmcnt(lgkm); 63 / 15 = do not wait for that counter
	void waitcnt(uint32_t vm, uint32_t lgkm)
	{
		sopp(SP_WAITCNT, (vm & 15u) | (7u << 4) | ((lgkm & 15u) << 8) | ((vm >> 4) & 3u) << 14);
	}
	void wait_lgkm() { waitcnt(63, 0); }
	void wait_vm(uint32_t n) { waitcnt(n, 15); }
	// a forward branch (s_branch / s_cbranch_*) whose distance `to` sets: returns its offset
	size_t fwd(uint32_t op)
	{
		const size_t at = b.size();
		sopp(op);
		return at;
	}
	// point the branch at byte offset `at` of the buffer to here
	void to(size_t at)
	{
		const uint32_t skip = (uint32_t)((b.size() - at - 4) / 4);
		b[at] = (uint8_t)skip;
		b[at + 1] = (uint8_t)(skip >> 8);
	}
	// a jump anywhere: to .Lcb + off, through the scratch pair s[60:61] (16 bytes)
	void long_jump(uint32_t off)
	{
		sop2(S2_ADD_U32, AH_S_JUNK, sreg(AH_S_CB), opnd{SRC_LIT, off});
		sop2(S2_ADDC_U32, AH_S_JUNK + 1, sreg(AH_S_CB + 1), opnd{128});
		sop1(S1_SETPC_B64, 0, sreg(AH_S_JUNK));
	}
};
