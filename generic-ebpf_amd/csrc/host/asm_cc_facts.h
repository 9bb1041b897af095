// asm_cc_facts.h — what the code generator knows while it compiles (asm_cc.cpp): the kernels'
// registers it names, the per-path facts about eBPF registers and stack words, and the family
// table.  Internal to asm_cc.cpp (one translation unit: everything here is file-local).
#pragma once
#include <algorithm>

#include "asm_handlers.h"
#include "internal.h"

#include "asm_cc.h"
#include "gfx950_enc.h"

namespace {

// ---------------------------------------------------------------- registers
// The kernels' registers this code names.  gen_abi.py assigns them and writes them into
// asm_handlers.h; these are aliases, so a register that moves there moves here with it.  (eBPF
// register rK in v[2K:2K+1] is the one convention both sides spell out: emitter::L / Hi.)
const int S_MODE = AH_S_MODE;          // the mode word (AH_MODE_* bits)
const int S_CB = AH_S_CB;              // s[4:5]: code base, routines are at S_CB + offset
const int S_OPND = AH_S_OPND;          // s10..s15: the operand words a handler body reads
const int S_SAVE = AH_S_SAVE;          // s[18:19]
const int S_DATA = AH_S_DATA;          // s[24:25]: dp_launch.data
const int S_STKSTRIDE = AH_S_STKSTRIDE;
const int S_PKTLDS = AH_S_PKTLDS;      // LDS offset of the wave's packet buffer
const int S_MASK = AH_S_MASK;          // s[48:49]: lanes argument of the fault routine, scratch
const int S_LINK = AH_S_LINK;          // s[50:51]: routine return address
const int S_CODE = AH_S_CODE;          // fault code argument
const int S_BYTES = AH_S_BYTES;        // .Lr_exit_k: the verdict bin
const int S_SHARED_HI = AH_S_SHARED + 1; // src_shared_base, high word
const int S_JUNK = AH_S_JUNK;          // s[60:61]: scratch pair, carry-out sink of v_mad_u64_u32
const int S_SHORT = AH_S_SHORT;        // s[74:75], general kernels: lanes with a packet below 64 B
const int PKT0 = AH_V_PKT0;            // the 16 staged packet dwords
const int V_PKT = AH_V_PKT;            // v[38:39]: packet address
const int V_LEN = AH_V_LEN;            // packet length
const int V_STK = AH_V_STK;            // lane stack bottom (LDS byte address)
const int V_L16 = AH_V_L16;            // staged kernels: lane * 16
const int V_RES = AH_V_RES;            // v[44:45]: r0 of retiring lanes
const int V_SEL = AH_V_SEL;            // 0x00010203 (byte reversal selector)
const int T0 = AH_V_H0, T1 = AH_V_H1, T2 = AH_V_H2, T3 = AH_V_H3; // handler temporaries

// ---------------------------------------------------------------- facts
struct rf {
	bool c = false;   // known constant
	uint64_t v = 0;
	uint8_t lz = 0;   // known leading zero bits (64 if c && v == 0)
	bool nz = false;  // known non-zero (a lookup that cannot fail)
	int8_t mp = -1;   // >= 0: a pointer to map mp's value number u32(r[mreg]) (+0)
	int8_t mreg = -1;
	int8_t hfwd = -1; // >= 0: a hashtable lookup result whose value's first 8 bytes register
	                  // hfwd's VGPRs hold (loaded with the probe, see AHF_HLOOKUP)
};

inline int
clz64(uint64_t x)
{
	return x ? __builtin_clzll(x) : 64;
}

inline rf
kconst(uint64_t v)
{
	rf r;
	r.c = true;
	r.v = v;
	r.lz = (uint8_t)clz64(v);
	r.nz = v != 0;
	return r;
}

inline rf
kbits(int bits)
{
	rf r;
	r.lz = (uint8_t)(bits <= 0 ? 64 : bits >= 64 ? 0 : 64 - bits);
	return r;
}

inline int
bits_of(const rf &r)
{
	return 64 - r.lz;
}

// a stack word whose bytes are the low `size` bytes of register `reg` (unchanged since)
struct sslot {
	uint32_t off; // LDS offset from the lane's stack bottom (the lowered operand)
	uint8_t size;
	int8_t reg;
};

struct facts {
	rf r[AH_NREGS];
	bool pv[AH_NREGS] = {}; // the register's VGPRs hold its value (false: a dead write skipped)
	sslot st[8];
	uint8_t nst = 0;

	// forget every fact that reads d's VGPRs through another name (self: also d's own, a map
	// pointer indexed by itself)
	void drop_aliases(int d, bool self)
	{
		uint8_t k = 0;
		for (uint8_t i = 0; i < nst; i++)
			if (st[i].reg != d)
				st[k++] = st[i];
		nst = k;
		for (int q = 0; q < AH_NREGS; q++) {
			if ((self || q != d) && r[q].mreg == d) {
				r[q].mp = -1;
				r[q].mreg = -1;
			}
			if (r[q].hfwd == d)
				r[q].hfwd = -1;
		}
	}
	void def(int d, const rf &v, bool phys = true)
	{
		r[d] = v;
		pv[d] = phys;
		drop_aliases(d, false);
	}
	// d's VGPRs are overwritten with something else while its value facts stay true (a register
	// dead from here on, reused as a scratch): nothing may read those VGPRs for d any more
	void clobber_phys(int d)
	{
		pv[d] = false;
		drop_aliases(d, true);
	}
	void store(uint32_t off, int size, int reg)
	{
		uint8_t k = 0;
		for (uint8_t i = 0; i < nst; i++)
			if (st[i].off + st[i].size <= off || off + (uint32_t)size <= st[i].off)
				st[k++] = st[i];
		nst = k;
		if (reg >= 0 && nst < 8)
			st[nst++] = sslot{off, (uint8_t)size, (int8_t)reg};
	}
	bool nofwd = false;
	bool t2zero = false; // v48 (T2) holds 0 in this path's lanes (the multiply addend's low word)
	const sslot *slot(uint32_t off, int size) const
	{
		if (nofwd)
			return nullptr;
		for (uint8_t i = 0; i < nst; i++)
			if (st[i].off == off && st[i].size >= size)
				return &st[i];
		return nullptr;
	}
};

struct mapinfo {
	uint64_t dev_base;
	uint32_t value_size, max_entries, lds_off;
};

// ---------------------------------------------------------------- families
// The generator (gen_abi.py) states each family's class and its index within the class
// (asm_handlers.h ah_fam_class / ah_fam_idx); nothing here depends on the order it registers them in.
inline int
class_of(int fam)
{
	return ah_fam_class[fam];
}

// access size in bytes of a load / store / counter family (its class index is log2 of it)
inline int
size_of(int fam)
{
	return 1 << ah_fam_idx[fam];
}

inline bool
is_cond_class(int cls)
{
	return cls == AHC_JR || cls == AHC_JI || cls == AHC_J32R || cls == AHC_J32I;
}

// the condition (AH_CC_*) of a conditional-jump family
inline int
cond_of(int fam)
{
	return ah_fam_idx[fam];
}

// the STX of a counter update, XADD (ebpf_gpu.h "Stores into map values"): generic stores
inline bool
is_value_store_class(int cls)
{
	return cls == AHC_CNTST || cls == AHC_XADD || cls == AHC_XADDF;
}

// a store through a pointer the compiler knows nothing about: it may hit the packet or the stack
inline bool
is_store_through_pointer(int cls)
{
	return cls == AHC_STXGEN || cls == AHC_STGEN || is_value_store_class(cls);
}

// the register a copied handler body writes (-1: none)
int
written_reg(int fam, int d)
{
	switch (class_of(fam)) {
	case AHC_LOOKUPSTK: case AHC_LOOKUPGEN: case AHC_HLOOKUP: case AHC_UPDATE: case AHC_HDELETE:
		return 0;
	case AHC_EXIT: case AHC_FAULT: case AHC_NOP:
	case AHC_STXGEN: case AHC_STXSTK: case AHC_STGEN: case AHC_STSTK:
	case AHC_CNTST: case AHC_XADD: case AHC_OVLINIT: case AHC_CNTAI: case AHC_CNTAL:
	case AHC_JR: case AHC_JI: case AHC_J32R: case AHC_J32I:
		return -1;
	default:
		return d < AH_NREGS ? d : -1;
	}
}

// registers a copied handler body reads
uint16_t
copied_uses(int fam, int d, int s)
{
	auto m = [](int r) -> uint16_t { return r < AH_NREGS ? (uint16_t)(1u << r) : 0; };
	switch (class_of(fam)) {
	case AHC_EXIT: return 1;
	case AHC_LOOKUPGEN: return (1u << 1) | (1u << 2);
	case AHC_HLOOKUP: case AHC_HDELETE: return 1u << 2;
	case AHC_UPDATE: return (1u << 2) | (1u << 3) | (1u << 4);
	case AHC_FAULT: case AHC_NOP: case AHC_LOOKUPSTK: case AHC_OVLINIT:
	case AHC_STSTK: case AHC_LDXPKTG: case AHC_LDXSTK: case AHC_LDXPKC:
		return 0;
	case AHC_MOV64R: return m(s);
	default:
		if (fam == AHF_A64I_MOV || fam == AHF_A32I_MOV)
			return 0;
		if (fam == AHF_A32R_MOV)
			return m(s);
		return m(d) | m(s); // (LDX*: s = the address; ST*: d = base, s = value; ALU: both)
	}
}

// facts for a copied body's result
rf
copied_result(int fam)
{
	switch (class_of(fam)) {
	case AHC_LDXGEN: case AHC_LDXMAP: case AHC_LDXPKTG: case AHC_LDXSTK: case AHC_LDXHV:
	case AHC_LDXPKC: case AHC_LDXPKTV:
		return size_of(fam) < 8 ? kbits(8 * size_of(fam)) : rf();
	case AHC_XADDF:
		return size_of(fam) == 4 ? kbits(32) : rf();
	case AHC_A32R: case AHC_A32I:
		return kbits(32);
	default:
		return rf();
	}
}

// operations with no effect besides writing their destination register (no fault, no memory
// write): skipped when the destination is dead
bool
pure_fam(int fam, bool specialised_map_load)
{
	switch (class_of(fam)) {
	case AHC_A64R: return fam != AHF_A64R_DIV && fam != AHF_A64R_MOD;
	case AHC_A32R: return fam != AHF_A32R_DIV && fam != AHF_A32R_MOD;
	case AHC_A64I: case AHC_A32I:
		return true; // immediate divisors are never zero here (the translator faults them)
	case AHC_BSWAP: case AHC_LDXPKC: case AHC_LDXSTK: case AHC_LOOKUPSTK:
		return true;
	case AHC_LDXMAP:
		return specialised_map_load;
	default:
		return false;
	}
}

// refine facts on the taken (taken = true) or fall-through edge of `d c K`
void
refine(facts &fa, int c, int d, uint64_t K, bool taken)
{
	rf &x = fa.r[d];
	if (x.c)
		return;
	if ((c == AH_CC_JEQ && taken) || (c == AH_CC_JNE && !taken)) {
		const bool keep_map = K != 0 && x.mp >= 0;
		rf k = kconst(K);
		if (keep_map) {
			k.mp = x.mp;
			k.mreg = x.mreg;
		}
		x = k;
		return;
	}
	if (K == 0 && ((c == AH_CC_JNE && taken) || (c == AH_CC_JEQ && !taken))) { // d != 0
		x.nz = true;
		return;
	}
	uint64_t B;
	bool ub = false;
	if ((c == AH_CC_JLE && taken) || (c == AH_CC_JGT && !taken)) { // d <= K (unsigned)
		B = K;
		ub = true;
	} else if (((c == AH_CC_JLT && taken) || (c == AH_CC_JGE && !taken)) && K) { // d < K
		B = K - 1;
		ub = true;
	}
	if (ub) {
		const int nb = 64 - clz64(B);
		if (64 - nb > x.lz)
			x.lz = (uint8_t)(64 - nb);
	}
}

} // namespace
