// asm_cc_emit.h — per-entry emission of the code generator (asm_cc.cpp): one emitter per lowered
// entry encodes the entry's family into its cc_block and updates the path's facts.  Internal to
// asm_cc.cpp.
#pragma once
#include "asm_cc_facts.h"

namespace {

// ---------------------------------------------------------------- per-entry emission
struct emitter {
	cc_block &blk;
	enc E;
	facts &f;
	const std::vector<mapinfo> &maps;
	uint16_t used = 0; // registers this entry's code reads

	emitter(cc_block &b, facts &fa, const std::vector<mapinfo> &m) : blk(b), E{b.body}, f(fa), maps(m) {}

	static int L(int r) { return 2 * r; }
	static int Hi(int r) { return 2 * r + 1; }
	bool hz(int r) const { return f.r[r].lz >= 32; }
	void use(int r) { used |= (uint16_t)(1u << r); }

	// LDXPKTV in the staged kernels: d = the z bytes at r_sr + K of the lane's packet.
	// * every running lane at the same offset (a cursor advanced by constants: C3L's header
	//   words): from the packet dwords v22..v37 the staging left in registers, indexed by the
	//   offset's dword (s_set_gpr_idx_on, M0) and aligned by its low bits — no memory access;
	// * otherwise, in keep mode (AH_MODE_KEEP: gpu_runtime.cpp sets it for staged launches of
	//   programs with these loads), from the wave's transposed LDS packet buffer (gen_emit.py
	//   lds_pkt_read) when every running lane's bytes lie in its 64;
	// * else the interpreter's handler body h (generic load, faults), spliced in by the code
	//   generator.
	// (The handler's own fast path re-derives the address from s[10:11] and tests the keep flag
	// first: here r_sr is read directly and K folds into the bounds.)
	void ldxpktv_staged(int d, int sr, int z, uint32_t K, int h)
	{
		const int S_U = S_JUNK, S_M = S_MASK;
		const int A = AH_V_H4, B = AH_V_H5, R0 = AH_V_R0, R1 = AH_V_R1, R2 = AH_V_R2;
		const uint32_t C = 64u - (uint32_t)z - K;            // last in-bounds offset T
		use(sr);
		E.vop2(V2_SUB_CO_U32, T2, vreg(L(sr)), V_PKT);               // T = r - pkt (64-bit)
		E.vop2(V2_SUBB_CO_U32, T3, vreg(Hi(sr)), V_PKT + 1);
		E.vop1(V1_READFIRSTLANE_B32, S_U, vreg(T2));
		E.vop1(V1_READFIRSTLANE_B32, S_U + 1, vreg(T3));
		E.vopc(VC_U64 + P_EQ, sreg(S_U), T2);                        // vcc = T == T(first lane)
		E.sop2(S2_ANDN2_B64, S_M, opnd{SRC_EXEC}, opnd{SRC_VCC});    // lanes that differ
		const size_t to_lds = E.fwd(SP_CBRANCH_SCC1);
		E.sopc(SC_CMP_LG_U32, S_U + 1, 128);                         // hi != 0
		const size_t slow0 = E.fwd(SP_CBRANCH_SCC1);
		E.sopc(SC_CMP_GT_U32, S_U, 128 + C);                         // lo > C
		const size_t slow1 = E.fwd(SP_CBRANCH_SCC1);
		if (K)
			E.sop2(S2_ADD_U32, S_U, sreg(S_U), opnd{128 + K});
		E.sop2(S2_LSHR_B32, S_U + 1, sreg(S_U), opnd{128 + 2});      // the dword index
		// (VOP3 sources are indexed too: profiles/r05/c3l_pktv/)
		E.sopc(SC_SET_GPR_IDX_ON, S_U + 1, 3);                       // (SRC0, SRC1)
		E.vop3(V3_ALIGNBYTE, L(d), VGPR0 + PKT0 + 1, VGPR0 + PKT0, (uint32_t)S_U);
		if (z == 8)
			E.vop3(V3_ALIGNBYTE, Hi(d), VGPR0 + PKT0 + 2, VGPR0 + PKT0 + 1, (uint32_t)S_U);
		E.sopp(SP_SET_GPR_IDX_OFF);
		if (z < 4)
			E.vop2(V2_AND, L(d), k32(z == 1 ? 0xffu : 0xffffu), L(d));
		if (z < 8)
			hi0(d);
		const size_t done0 = E.fwd(SP_BRANCH);                       // (patched past the splice)
		E.to(to_lds);
		E.sopc(SC_BITCMP1_B32, S_MODE, 128 + AH_MODE_KEEP);          // s_bitcmp1_b32 s7, 14
		const size_t slow2 = E.fwd(SP_CBRANCH_SCC0);                 // no keep mode: the handler
		E.vopc(VC_U64 + P_GE, k32(C), T2);                           // vcc = T <= C
		E.sop2(S2_ANDN2_B64, S_JUNK, opnd{SRC_EXEC}, opnd{SRC_VCC}); // lanes out
		const size_t slow3 = E.fwd(SP_CBRANCH_SCC1);
		E.vop2(V2_LSHRREV_B32, A, opnd{128 + 2}, V_L16);             // A = S_PKTLDS + 4 lane
		E.vop2(V2_ADD_U32, A, sreg(S_PKTLDS), A);
		if (K)
			E.vop2(V2_ADD_U32, T2, k32(K), T2);                  // T += K (<= 64 - z)
		E.vop2(V2_LSHRREV_B32, B, opnd{128 + 2}, T2);                // B = A + 256 (T >> 2)
		E.vop3(V3_LSHL_ADD_U32, B, VGPR0 + B, 128 + 8, VGPR0 + A);
		if (z == 1)
			E.ds(DS_READ_B32, B, 0, 0, R0, 0);
		else
			E.ds(DS_READ2_B32, B, 0, 0, R0, 0, 64);
		if (z == 8)
			E.ds(DS_READ_B32, B, 0, 0, R2, 0x200 & 0xff, 0x200 >> 8);
		E.wait_lgkm();
		E.vop3(V3_ALIGNBYTE, L(d), VGPR0 + (z == 1 ? R0 : R1), VGPR0 + R0, VGPR0 + T2);
		if (z == 8)
			E.vop3(V3_ALIGNBYTE, Hi(d), VGPR0 + R2, VGPR0 + R1, VGPR0 + T2);
		else if (z < 4)
			E.vop2(V2_AND, L(d), k32(z == 1 ? 0xffu : 0xffffu), L(d));
		loaded(d, z);
		const size_t done1 = E.fwd(SP_BRANCH);                       // (patched past the splice)
		// the slow branches, and both done branches, to the body's end: the splice starts there,
		// and the code generator moves the done branches past it
		for (size_t at : {slow0, slow1, slow2, slow3, done0, done1})
			E.to(at);
		blk.splice_h = h;
		blk.splice_at = (uint32_t)E.b.size();
		blk.splice_br[0] = (uint32_t)done0;
		blk.splice_br[1] = (uint32_t)done1;
		blk.splice_sval[0] = K;
		blk.splice_sval[1] = 0;
		f.t2zero = false;
	}
	// an SGPR holding the 32-bit constant v for this body (s13, s14, s15)
	uint32_t sconst(uint32_t v)
	{
		for (int k = 3; k < 6; k++)
			if ((blk.reads & (1u << k)) && blk.sval[k] == v)
				return (uint32_t)(S_OPND + k);
		for (int k = 3; k < 6; k++)
			if (!(blk.reads & (1u << k))) {
				blk.reads |= (uint8_t)(1u << k);
				blk.sval[k] = v;
				return (uint32_t)(S_OPND + k);
			}
		return UINT32_MAX; // never: no body needs four constants
	}
	// the SGPR pair s[10:11] holding the 64-bit constant v
	uint32_t spair(uint64_t v)
	{
		blk.reads |= 3;
		blk.sval[0] = (uint32_t)v;
		blk.sval[1] = (uint32_t)(v >> 32);
		return (uint32_t)S_OPND;
	}
	uint32_t c3(uint32_t v)
	{
		uint32_t c;
		if (inline_i64((int64_t)(int32_t)v, &c))
			return c;
		return sconst(v);
	}
	// a 32-bit constant as a VOP3 source that does not use the constant bus: an inline
	// constant, or the literal moved into VGPR `tmp` first (for an instruction that already reads
	// an SGPR)
	uint32_t vconst(uint32_t v, int tmp)
	{
		uint32_t c;
		if (inline_i64((int64_t)(int32_t)v, &c))
			return c;
		mov32(tmp, v);
		return VGPR0 + (uint32_t)tmp;
	}
	uint32_t c64(uint64_t v)
	{
		uint32_t c;
		if (inline_i64((int64_t)v, &c))
			return c;
		return spair(v);
	}

	void mov32(int vd, uint32_t v) { E.vop1(V1_MOV_B32, vd, k32(v)); }
	// hi(d) = 0 after a write of lo(d) (d's previous value read or not)
	void hi0(int d)
	{
		if (!(f.pv[d] && hz(d)))
			mov32(Hi(d), 0);
	}
	// d holds a load of z bytes: its VGPRs are written, but for the high word of one below 8 bytes
	void loaded(int d, int z)
	{
		if (z < 8)
			hi0(d);
		f.def(d, z < 8 ? kbits(8 * z) : rf());
	}
	// LDS load of z bytes at [v(addr) + off] into v(vd) (v[vd:vd+1]), waited for
	void ds_read(int z, int addr, int vd, uint32_t off)
	{
		if (z == 8)
			E.ds(DS_READ2_B32, addr, 0, 0, vd, off / 4, off / 4 + 1);
		else
			E.ds(z == 4 ? DS_READ_B32 : z == 2 ? DS_READ_U16 : DS_READ_U8, addr, 0, 0, vd, off);
		E.wait_lgkm();
	}
	// d = v (a constant), skipping halves the registers already hold
	void mov64(int d, uint64_t v)
	{
		const rf &o = f.r[d];
		const bool pv = f.pv[d];
		const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
		if (!(pv && o.c && (uint32_t)o.v == lo))
			mov32(L(d), lo);
		if (!(pv && ((o.c && (uint32_t)(o.v >> 32) == hi) || (hi == 0 && hz(d)))))
			mov32(Hi(d), hi);
		f.def(d, kconst(v));
	}
	// d = s (registers)
	void copy64(int d, int s)
	{
		if (d == s) {
			use(s);
			return;
		}
		if (f.r[s].c) {
			mov64(d, f.r[s].v);
			return;
		}
		use(s);
		if (hz(s)) {
			E.vop1(V1_MOV_B32, L(d), vreg(L(s)));
			hi0(d);
		} else {
			E.vop1(V1_MOV_B64, L(d), vreg(L(s)));
		}
		rf v = f.r[s];
		v.mp = -1; // (keep it simple: provenance stays with the original)
		v.mreg = -1;
		f.def(d, v);
	}

	// ---- ALU64 with a constant operand (d op= K)
	void add64i(int d, uint64_t K)
	{
		const rf x = f.r[d];
		if (K == 0) {
			use(d); // (a no-op passes d's value through)
			return;
		}
		if (x.c) {
			mov64(d, x.v + K);
			return;
		}
		use(d);
		E.vop3(V3_LSHL_ADD_U64, L(d), c64(K), 128, VGPR0 + L(d));
		f.def(d, (int64_t)K >= 0 ? kbits(std::max(bits_of(x), 64 - clz64(K)) + 1) : rf());
	}
	void or64i(int d, uint64_t K)
	{
		const rf x = f.r[d];
		if (x.c) {
			mov64(d, x.v | K);
			return;
		}
		if (K == 0) {
			use(d);
			return;
		}
		use(d);
		const uint32_t lo = (uint32_t)K, hi = (uint32_t)(K >> 32);
		if (lo)
			E.vop2(V2_OR, L(d), k32(lo), L(d));
		if (hi == 0xffffffffu)
			mov32(Hi(d), hi);
		else if (hi)
			E.vop2(V2_OR, Hi(d), k32(hi), Hi(d));
		rf v = kbits(std::max(bits_of(x), 64 - clz64(K)));
		v.nz = true;
		f.def(d, v);
	}
	void xor64i(int d, uint64_t K)
	{
		const rf x = f.r[d];
		if (x.c) {
			mov64(d, x.v ^ K);
			return;
		}
		if (K == 0) {
			use(d);
			return;
		}
		use(d);
		const uint32_t lo = (uint32_t)K, hi = (uint32_t)(K >> 32);
		if (lo)
			E.vop2(V2_XOR, L(d), k32(lo), L(d));
		if (hi)
			E.vop2(V2_XOR, Hi(d), k32(hi), Hi(d));
		f.def(d, kbits(std::max(bits_of(x), 64 - clz64(K))));
	}
	void and64i(int d, uint64_t K)
	{
		const rf x = f.r[d];
		if (x.c) {
			mov64(d, x.v & K);
			return;
		}
		if (K == ~0ull) {
			use(d);
			return;
		}
		if (K == 0) {
			mov64(d, 0);
			return;
		}
		use(d);
		const uint32_t lo = (uint32_t)K, hi = (uint32_t)(K >> 32);
		if (lo == 0)
			mov32(L(d), 0);
		else if (lo != 0xffffffffu)
			E.vop2(V2_AND, L(d), k32(lo), L(d));
		if (hi == 0)
			hi0(d);
		else if (hi != 0xffffffffu && !hz(d))
			E.vop2(V2_AND, Hi(d), k32(hi), Hi(d));
		f.def(d, kbits(std::min(bits_of(x), 64 - clz64(K))));
	}
	void lsh64i(int d, uint32_t c)
	{
		c &= 63;
		const rf x = f.r[d];
		if (c == 0) {
			use(d);
			return;
		}
		if (x.c) {
			mov64(d, x.v << c);
			return;
		}
		use(d);
		const int nb = std::min(64, bits_of(x) + (int)c);
		if (c >= 32) {
			if (c == 32)
				E.vop1(V1_MOV_B32, Hi(d), vreg(L(d)));
			else
				E.vop2(V2_LSHLREV_B32, Hi(d), opnd{128 + (c - 32)}, L(d));
			mov32(L(d), 0);
		} else if (nb <= 32) {
			E.vop2(V2_LSHLREV_B32, L(d), opnd{128 + c}, L(d));
		} else {
			E.vop3(V3_LSHLREV_B64, L(d), 128 + c, VGPR0 + L(d), 0);
		}
		f.def(d, kbits(nb));
	}
	void rsh64i(int d, uint32_t c)
	{
		c &= 63;
		const rf x = f.r[d];
		if (c == 0) {
			use(d);
			return;
		}
		if (x.c) {
			mov64(d, x.v >> c);
			return;
		}
		const int nb = std::max(0, bits_of(x) - (int)c);
		if (nb == 0) {
			mov64(d, 0);
			return;
		}
		use(d);
		if (c >= 32) {
			if (c == 32)
				E.vop1(V1_MOV_B32, L(d), vreg(Hi(d)));
			else
				E.vop2(V2_LSHRREV_B32, L(d), opnd{128 + (c - 32)}, Hi(d));
			mov32(Hi(d), 0);
		} else if (hz(d)) {
			E.vop2(V2_LSHRREV_B32, L(d), opnd{128 + c}, L(d));
		} else {
			E.vop3(V3_LSHRREV_B64, L(d), 128 + c, VGPR0 + L(d), 0);
		}
		f.def(d, kbits(nb));
	}
	void mul64i(int d, uint64_t K)
	{
		const rf x = f.r[d];
		if (x.c) {
			mov64(d, x.v * K);
			return;
		}
		if (K == 0) {
			mov64(d, 0);
			return;
		}
		if (K == 1) {
			use(d);
			return;
		}
		if ((K & (K - 1)) == 0) {
			lsh64i(d, (uint32_t)__builtin_ctzll(K));
			return;
		}
		use(d);
		const int nb = std::min(64, bits_of(x) + 64 - clz64(K));
		const uint32_t lo = (uint32_t)K, hi = (uint32_t)(K >> 32);
		const uint32_t klo = c3(lo);
		// d * K mod 2^64 = lo(d) * lo(K) + ((hi(d) * lo(K) + lo(d) * hi(K)) << 32): the cross
		// terms (low words only) go into the high word of the addend v[48:49] = {0, cross} of
		// one v_mad_u64_u32 that writes d in place
		if (hz(d) && hi == 0) {
			E.vop3(V3_MAD_U64_U32, L(d), VGPR0 + L(d), klo, 128, S_JUNK);
			f.def(d, kbits(nb));
			return;
		}
		if (!f.t2zero) {
			mov32(T2, 0);
			f.t2zero = true;
		}
		if (hi == 0) {
			E.vop3(V3_MUL_LO_U32, T3, VGPR0 + Hi(d), klo, 0);
		} else if (hz(d)) {
			E.vop3(V3_MUL_LO_U32, T3, VGPR0 + L(d), c3(hi), 0);
		} else {
			E.vop3(V3_MUL_LO_U32, T3, VGPR0 + Hi(d), klo, 0);
			E.vop3(V3_MUL_LO_U32, T1, VGPR0 + L(d), c3(hi), 0);
			E.vop2(V2_ADD_U32, T3, vreg(T3), T1);
		}
		E.vop3(V3_MAD_U64_U32, L(d), VGPR0 + L(d), klo, VGPR0 + T2, S_JUNK);
		f.def(d, kbits(nb));
	}

	// ---- ALU32 (lo op= k; hi = 0)
	// src >= 0: the operand is u32(r[src]) instead of r[d] (a 32-bit MOV d = src fused into
	// this operation by the caller)
	bool alu32i(int fam, int d, uint32_t k, int src = -1)
	{
		const int sr = src >= 0 ? src : d;
		const rf x = f.r[sr];
		const uint32_t a = (uint32_t)x.v;
		const int ab = std::min(32, bits_of(x));
		if (x.c || fam == AHF_A32I_MOV) {
			uint32_t r;
			switch (fam) {
			case AHF_A32I_ADD: r = a + k; break;
			case AHF_A32I_SUB: r = a - k; break;
			case AHF_A32I_MUL: r = a * k; break;
			case AHF_A32I_OR: r = a | k; break;
			case AHF_A32I_AND: r = a & k; break;
			case AHF_A32I_XOR: r = a ^ k; break;
			case AHF_A32I_LSH: r = a << (k & 31); break;
			case AHF_A32I_RSH: r = a >> (k & 31); break;
			case AHF_A32I_MOV: r = k; break;
			default: return false;
			}
			mov64(d, r);
			return true;
		}
		int nb = 32;
		const size_t at = blk.body.size();
		switch (fam) {
		case AHF_A32I_ADD:
			if (k)
				E.vop2(V2_ADD_U32, L(d), k32(k), L(sr));
			nb = k ? std::min(32, std::max(ab, 32 - __builtin_clz(k)) + 1) : ab;
			break;
		case AHF_A32I_SUB:
			if (k)
				E.vop2(V2_SUBREV_U32, L(d), k32(k), L(sr));
			nb = k ? 32 : ab;
			break;
		case AHF_A32I_MUL:
			E.vop3(V3_MUL_LO_U32, L(d), VGPR0 + L(sr), c3(k), 0);
			nb = k ? std::min(32, ab + 32 - __builtin_clz(k)) : 0;
			break;
		case AHF_A32I_OR:
			if (k)
				E.vop2(V2_OR, L(d), k32(k), L(sr));
			nb = std::max(ab, k ? 32 - __builtin_clz(k) : 0);
			break;
		case AHF_A32I_AND:
			if (k != 0xffffffffu)
				E.vop2(V2_AND, L(d), k32(k), L(sr));
			nb = std::min(ab, k ? 32 - __builtin_clz(k) : 0);
			break;
		case AHF_A32I_XOR:
			if (k)
				E.vop2(V2_XOR, L(d), k32(k), L(sr));
			nb = std::max(ab, k ? 32 - __builtin_clz(k) : 0);
			break;
		case AHF_A32I_LSH:
			if (k & 31)
				E.vop2(V2_LSHLREV_B32, L(d), opnd{128 + (k & 31)}, L(sr));
			nb = std::min(32, ab + (int)(k & 31));
			break;
		case AHF_A32I_RSH:
			if (k & 31)
				E.vop2(V2_LSHRREV_B32, L(d), opnd{128 + (k & 31)}, L(sr));
			nb = std::max(0, ab - (int)(k & 31));
			break;
		default:
			return false;
		}
		if (sr != d && blk.body.size() == at) // (an identity operation: the fused copy alone)
			E.vop1(V1_MOV_B32, L(d), vreg(L(sr)));
		use(sr);
		hi0(d);
		f.def(d, kbits(nb));
		return true;
	}
	bool alu32r(int fam, int d, int s)
	{
		if (f.r[s].c) { // the same operation with an immediate operand
			switch (fam) {
			case AHF_A32R_ADD: return alu32i(AHF_A32I_ADD, d, (uint32_t)f.r[s].v);
			case AHF_A32R_SUB: return alu32i(AHF_A32I_SUB, d, (uint32_t)f.r[s].v);
			case AHF_A32R_MUL: return alu32i(AHF_A32I_MUL, d, (uint32_t)f.r[s].v);
			case AHF_A32R_OR: return alu32i(AHF_A32I_OR, d, (uint32_t)f.r[s].v);
			case AHF_A32R_AND: return alu32i(AHF_A32I_AND, d, (uint32_t)f.r[s].v);
			case AHF_A32R_XOR: return alu32i(AHF_A32I_XOR, d, (uint32_t)f.r[s].v);
			case AHF_A32R_LSH: return alu32i(AHF_A32I_LSH, d, (uint32_t)f.r[s].v);
			case AHF_A32R_RSH: return alu32i(AHF_A32I_RSH, d, (uint32_t)f.r[s].v);
			case AHF_A32R_MOV: return alu32i(AHF_A32I_MOV, d, (uint32_t)f.r[s].v);
			default: break; // (DIV, MOD: the handler body)
			}
		}
		const rf x = f.r[d];
		const int ab = std::min(32, bits_of(x)), sb = std::min(32, bits_of(f.r[s]));
		int nb = 32;
		switch (fam) {
		case AHF_A32R_ADD: E.vop2(V2_ADD_U32, L(d), vreg(L(d)), L(s)); nb = std::min(32, std::max(ab, sb) + 1); break;
		case AHF_A32R_SUB: E.vop2(V2_SUB_U32, L(d), vreg(L(d)), L(s)); break;
		case AHF_A32R_MUL: E.vop3(V3_MUL_LO_U32, L(d), VGPR0 + L(d), VGPR0 + L(s), 0); nb = std::min(32, ab + sb); break;
		case AHF_A32R_OR: E.vop2(V2_OR, L(d), vreg(L(s)), L(d)); nb = std::max(ab, sb); break;
		case AHF_A32R_AND: E.vop2(V2_AND, L(d), vreg(L(s)), L(d)); nb = std::min(ab, sb); break;
		case AHF_A32R_XOR: E.vop2(V2_XOR, L(d), vreg(L(s)), L(d)); nb = std::max(ab, sb); break;
		case AHF_A32R_LSH: E.vop2(V2_LSHLREV_B32, L(d), vreg(L(s)), L(d)); break;
		case AHF_A32R_RSH: E.vop2(V2_LSHRREV_B32, L(d), vreg(L(s)), L(d)); nb = ab; break;
		case AHF_A32R_MOV: E.vop1(V1_MOV_B32, L(d), vreg(L(s))); nb = sb; break;
		default: return false;
		}
		use(s);
		if (fam != AHF_A32R_MOV)
			use(d);
		if (d == s && (fam == AHF_A32R_SUB || fam == AHF_A32R_XOR))
			nb = 0;
		hi0(d);
		f.def(d, kbits(nb));
		return true;
	}
	bool alu64r(int fam, int d, int s)
	{
		const rf xs = f.r[s];
		const rf x = f.r[d];
		if (d == s) {
			switch (fam) {
			case AHF_A64R_ADD: lsh64i(d, 1); return true;
			case AHF_A64R_SUB: case AHF_A64R_XOR: mov64(d, 0); return true;
			case AHF_A64R_OR: case AHF_A64R_AND: use(d); return true;
			default: return false;
			}
		}
		if (xs.c) {
			switch (fam) {
			case AHF_A64R_ADD: add64i(d, xs.v); return true;
			case AHF_A64R_SUB: add64i(d, 0 - xs.v); return true;
			case AHF_A64R_MUL: mul64i(d, xs.v); return true;
			case AHF_A64R_OR: or64i(d, xs.v); return true;
			case AHF_A64R_AND: and64i(d, xs.v); return true;
			case AHF_A64R_XOR: xor64i(d, xs.v); return true;
			case AHF_A64R_LSH: lsh64i(d, (uint32_t)xs.v); return true;
			case AHF_A64R_RSH: rsh64i(d, (uint32_t)xs.v); return true;
			default: return false;
			}
		}
		if (x.c && x.v == 0 && (fam == AHF_A64R_ADD || fam == AHF_A64R_OR || fam == AHF_A64R_XOR)) {
			copy64(d, s);
			return true;
		}
		switch (fam) {
		case AHF_A64R_ADD:
			use(d);
			use(s);
			E.vop3(V3_LSHL_ADD_U64, L(d), VGPR0 + L(s), 128, VGPR0 + L(d));
			f.def(d, kbits(std::min(64, std::max(bits_of(x), bits_of(xs)) + 1)));
			return true;
		case AHF_A64R_OR:
		case AHF_A64R_XOR: {
			use(d);
			use(s);
			const uint32_t op = fam == AHF_A64R_OR ? V2_OR : V2_XOR;
			E.vop2(op, L(d), vreg(L(s)), L(d));
			if (!hz(s))
				E.vop2(op, Hi(d), vreg(Hi(s)), Hi(d));
			f.def(d, kbits(std::max(bits_of(x), bits_of(xs))));
			return true;
		}
		case AHF_A64R_AND:
			use(d);
			use(s);
			E.vop2(V2_AND, L(d), vreg(L(s)), L(d));
			if (hz(s))
				hi0(d);
			else if (!hz(d))
				E.vop2(V2_AND, Hi(d), vreg(Hi(s)), Hi(d));
			f.def(d, kbits(std::min(bits_of(x), bits_of(xs))));
			return true;
		default:
			return false;
		}
	}

	// ---- byte swaps (BE16/BE32 zero-extend; LE is lowered to AND)
	bool bswap(int fam, int d)
	{
		if (fam == AHF_BSWAP64)
			return false;
		const bool w16 = fam == AHF_BSWAP16;
		const rf x = f.r[d];
		if (x.c) {
			mov64(d, w16 ? __builtin_bswap16((uint16_t)x.v) : __builtin_bswap32((uint32_t)x.v));
			return true;
		}
		use(d);
		E.vop3(V3_PERM_B32, L(d), 128, VGPR0 + L(d), w16 ? sconst(0x0c0c0001u) : VGPR0 + V_SEL);
		hi0(d);
		f.def(d, kbits(w16 ? 16 : 32));
		return true;
	}

	// ---- staged packet load at constant offset `off`, size z; swap_bytes = 0, 2 or 4 (a fused
	// BE16 / BE32 of the loaded register)
	// General kernels with header staging: the packet load at constant offset off < 64 from the
	// staged header registers, like the handler (h_ldx_pkt_const) but with its two per-load lane
	// compares replaced by one per-group mask: s[74:75] = lanes whose packet is shorter than 64
	// bytes (set by the prologue).  Only such lanes can fault (off + z > len) or need the load
	// from memory; when none is running the load is the extract alone.
	void ldxpkc_general(int d, int z, int off, uint32_t fault_off)
	{
		E.sop2(S2_AND_B64, S_MASK, sreg(S_SHORT), opnd{SRC_EXEC});       // (scc)
		const size_t to_fast = E.fwd(SP_CBRANCH_SCC0);
		fault_past(off + z, fault_off);
		const facts f0 = f; // (both paths emit the same extract from the same facts)
		ldxpkc(d, z, off, 0);
		E.sop2(S2_AND_B64, S_MASK, sreg(S_SHORT), opnd{SRC_EXEC});
		const size_t to_end1 = E.fwd(SP_CBRANCH_SCC0);
		E.sop1(S1_MOV_B64, S_JUNK, opnd{SRC_EXEC});
		E.sop1(S1_MOV_B64, SRC_EXEC, sreg(S_MASK));                      // exec = short lanes
		E.global_load(__builtin_ctz(z), L(d), V_PKT, (uint32_t)off);
		E.wait_vm(0);
		if (z < 8)
			mov32(Hi(d), 0);
		E.sop1(S1_MOV_B64, SRC_EXEC, sreg(S_JUNK));                      // exec back
		const size_t to_end2 = E.fwd(SP_BRANCH);
		E.to(to_fast);
		f = f0;
		ldxpkc(d, z, off, 0);
		E.to(to_end1);
		E.to(to_end2);
	}
	// MEM-fault the running lanes whose packet is shorter than `end` (s[48:49] = those lanes)
	void fault_past(uint32_t end, uint32_t fault_off)
	{
		E.vopc(VC_U32 + P_GT, k32(end), V_LEN);                          // vcc = end > len
		E.sop2(S2_AND_B64, S_MASK, opnd{SRC_VCC}, opnd{SRC_EXEC});
		E.sopp(SP_CBRANCH_SCC0, 5);                                      // over the 5 dwords below
		E.sop1(S1_MOV_B32, S_CODE, opnd{128 + 3});                       // s52 = 3 (MEM)
		call_routine(fault_off, 0);                                      // (4 dwords)
	}
	void ldxpkc(int d, int z, int off, int swap_bytes)
	{
		const int k = off >> 2, sh = off & 3;
		const int lo = PKT0 + k, nx = PKT0 + (k + 1 < 16 ? k + 1 : k);
		if (swap_bytes) {
			// result byte i = packet byte off + (W-1-i) for W-1-i < z
			uint32_t sel = 0;
			for (int i = 0; i < 4; i++) {
				const int j = swap_bytes - 1 - i;
				const uint32_t b = (i < swap_bytes && j < z) ? (uint32_t)(sh + j) : 0x0cu;
				sel |= b << (8 * i);
			}
			const uint32_t sc = sel == 0x00010203u ? VGPR0 + V_SEL : sconst(sel);
			E.vop3(V3_PERM_B32, L(d), VGPR0 + nx, VGPR0 + lo, sc);
			hi0(d);
			// (the loaded bytes land at the top of the swapped word: a byte under BE32 is b << 24,
			// so the value needs all 8 * W bits, not 8 * z)
			f.def(d, kbits(8 * swap_bytes));
			return;
		}
		if (z == 1) {
			E.vop3(V3_BFE_U32, L(d), VGPR0 + lo, 128 + 8 * sh, 128 + 8);
		} else if (z == 2) {
			if (sh <= 2)
				E.vop3(V3_BFE_U32, L(d), VGPR0 + lo, 128 + 8 * sh, 128 + 16);
			else
				E.vop3(V3_PERM_B32, L(d), VGPR0 + nx, VGPR0 + lo, sconst(0x0c0c0403u));
		} else if (z == 4) {
			if (sh == 0)
				E.vop1(V1_MOV_B32, L(d), vreg(lo));
			else
				E.vop3(V3_ALIGNBYTE, L(d), VGPR0 + nx, VGPR0 + lo, 128 + sh);
		} else {
			if (sh == 0) {
				if ((lo & 1) == 0) {
					E.vop1(V1_MOV_B64, L(d), vreg(lo));
				} else {
					E.vop1(V1_MOV_B32, L(d), vreg(lo));
					E.vop1(V1_MOV_B32, Hi(d), vreg(lo + 1));
				}
			} else {
				E.vop3(V3_ALIGNBYTE, L(d), VGPR0 + lo + 1, VGPR0 + lo, 128 + sh);
				E.vop3(V3_ALIGNBYTE, Hi(d), VGPR0 + lo + 2, VGPR0 + lo + 1, 128 + sh);
			}
		}
		loaded(d, z);
	}

	// ---- stack accesses at a known LDS offset `o` from the lane's stack bottom
	void stxstk(int z, int r, uint32_t o)
	{
		use(r);
		if (z == 8)
			E.ds(DS_WRITE2_B32, V_STK, L(r), Hi(r), 0, o / 4, o / 4 + 1);
		else
			E.ds(z == 4 ? DS_WRITE_B32 : z == 2 ? DS_WRITE_B16 : DS_WRITE_B8, V_STK, L(r), 0, 0, o);
		f.store(o, z, r);
	}
	// low z bytes of register s into d
	void low_bytes(int d, int s, int z)
	{
		if (z == 8) {
			copy64(d, s);
			return;
		}
		const rf xs = f.r[s];
		if (xs.c) {
			mov64(d, z == 4 ? (uint32_t)xs.v : xs.v & ((1ull << (8 * z)) - 1));
			return;
		}
		use(s);
		const int sb = std::min(bits_of(xs), 8 * z);
		if (bits_of(xs) <= 8 * z || z == 4)
			E.vop1(V1_MOV_B32, L(d), vreg(L(s)));
		else
			E.vop2(V2_AND, L(d), k32(z == 1 ? 0xffu : 0xffffu), L(s));
		hi0(d);
		f.def(d, kbits(sb));
	}
	void ldxstk(int z, int d, uint32_t o)
	{
		if (const sslot *sl = f.slot(o, z)) {
			low_bytes(d, sl->reg, z);
			return;
		}
		blk.stack_read = true;
		ds_read(z, V_STK, L(d), o);
		loaded(d, z);
	}

	// ---- array-map lookup resolved to map `mi` with the key at stack offset `o`: specialised
	// when the key is a register proven below max_entries (the lookup cannot return NULL)
	bool lookup_stk(int mi, uint32_t o)
	{
		if (mi < 0)
			return false;
		const mapinfo &m = maps[mi];
		const sslot *sl = f.slot(o, 4);
		if (!sl)
			return false;
		const int R = sl->reg;
		const rf xr = f.r[R];
		const uint64_t kmax = xr.c ? (uint32_t)xr.v : (bits_of(xr) >= 32 ? 0xffffffffull : (1ull << bits_of(xr)) - 1);
		if (kmax >= m.max_entries || m.max_entries > (1u << 24))
			return false;
		use(R);
		// (the map base is an SGPR pair: the value size must not be a second SGPR)
		E.vop3(V3_MAD_U64_U32, L(0), VGPR0 + L(R), vconst(m.value_size, T0), spair(m.dev_base), S_JUNK);
		rf v;
		v.nz = true;
		v.mp = (int8_t)mi;
		v.mreg = (int8_t)R;
		f.def(0, v);
		return true;
	}
	// LDXHV through a non-NULL hashtable lookup result whose value's first 8 bytes were
	// loaded with the probe into register D's VGPRs: an extract, no memory access
	bool ldxhv_fwd(int z, int d, int s, int32_t o)
	{
		const rf xs = f.r[s];
		if (xs.hfwd < 0 || !xs.nz || o < 0 || o + z > 8 || (o % z) != 0)
			return false;
		const int D = xs.hfwd;
		use(s);
		use(D);
		if (z == 8) {
			if (d != D)
				E.vop1(V1_MOV_B64, L(d), vreg(L(D)));
		} else if (z == 4) {
			E.vop1(V1_MOV_B32, L(d), vreg(L(D) + o / 4));
		} else {
			E.vop3(V3_BFE_U32, L(d), VGPR0 + L(D) + (uint32_t)(o / 4), 128 + 8 * (uint32_t)(o % 4),
			       128 + 8 * (uint32_t)z);
		}
		if (z < 8)
			mov32(Hi(d), 0);
		f.def(d, z == 8 ? rf() : kbits(8 * z));
		return true;
	}
	// LDXMAP through a pointer with known map and index register: the LDS copy, no check
	bool ldxmap(int z, int d, int s, uint64_t imm)
	{
		const rf xs = f.r[s];
		if (xs.mp < 0 || xs.mreg < 0 || !xs.nz)
			return false;
		const mapinfo &m = maps[xs.mp];
		if (m.lds_off == ~0u)
			return false;
		const int64_t c = (int64_t)(m.dev_base - imm); // the access offset within the value
		if (c < 0 || c + z > (int64_t)m.value_size)
			return false;
		const int R = xs.mreg;
		use(R);
		const uint32_t base = m.lds_off + (uint32_t)c;
		// (base >= the map area's LDS offset is never an inline constant: an SGPR, so a value
		// size that is none either goes through a VGPR)
		E.vop3(V3_MAD_U32_U24, T0, VGPR0 + L(R), vconst(m.value_size, T1), c3(base));
		ds_read(z, T0, L(d), 0);
		loaded(d, z);
		return true;
	}

	// ---- EXIT with r0 known: result and verdict bin set here, then .Lr_exit_k (gen_routines.py)
	void exit_known(uint64_t r0, uint32_t exitk_off, bool call)
	{
		mov32(V_RES, (uint32_t)r0);
		mov32(V_RES + 1, (uint32_t)(r0 >> 32));
		if (call) {
			// structured programs: the verdict count inline (.Lr_exit_k's work): one LDS add
			// of popcount(exec) to bin min(r0, 255); the exiting lanes leave the alive mask
			// (lane 0's V_L16 = 0 addresses the bin through the instruction offset; the alive
			// mask is not read again before the group ends in a structured program)
			const int R8 = AH_V_R8;
			const uint32_t bin = r0 < 255 ? (uint32_t)r0 : 255u;
			E.sop1(S1_BCNT1_I32_B64, S_CODE, opnd{SRC_EXEC});
			E.sop1(S1_MOV_B64, S_SAVE, opnd{SRC_EXEC});
			E.sop1(S1_MOV_B64, SRC_EXEC, opnd{128 + 1});                   // exec = lane 0
			E.vop1(V1_MOV_B32, R8, sreg(S_CODE));
			E.ds(DS_ADD_U32, V_L16, R8, 0, 0, (bin * 4) & 0xff, (bin * 4) >> 8);
			E.sop1(S1_MOV_B64, SRC_EXEC, sreg(S_SAVE));
			(void)exitk_off;
			return;
		}
		E.sop1(S1_MOV_B32, S_BYTES, k32(r0 < 255 ? (uint32_t)r0 : 255u));
		E.long_jump(exitk_off);
	}
	// EXIT with r0 in registers (structured programs), inline: r0 into the result slot and one
	// LDS histogram add per lane at bin min(r0, 255) (what .Lr_exit does, without the call,
	// the return and the uniform-verdict test)
	void exit_inline()
	{
		const int R8 = AH_V_R8, R9 = AH_V_R9;
		use(0);
		E.vop1(V1_MOV_B32, V_RES, vreg(0));
		E.vop1(V1_MOV_B32, V_RES + 1, vreg(1));
		int bin = 0; // v0 holds the bin if r0 < 256
		if (f.r[0].lz < 56) {
			E.vop1(V1_MOV_B32, R8, k32(255));
			E.vop1(V1_MOV_B32, R9, opnd{128});
			E.vopc(VC_U64 + P_LT, vreg(0), R8);            // vcc = r0 < 255
			E.vop2(V2_CNDMASK_B32, R8, vreg(R8), 0);       // v60 = vcc ? v0 : v60
			bin = R8;
		}
		E.vop2(V2_LSHLREV_B32, R8, opnd{128 + 2}, bin);
		E.vop1(V1_MOV_B32, R9, opnd{128 + 1});
		E.ds(DS_ADD_U32, R8, R9, 0, 0, 0);
	}
	// call a routine that returns (structured programs): the link pair s[50:51]
	void call_routine(uint32_t off, uint16_t reads)
	{
		used |= reads;
		E.sop2(S2_ADD_U32, S_LINK, sreg(S_CB), opnd{SRC_LIT, off});
		E.sop2(S2_ADDC_U32, S_LINK + 1, sreg(S_CB + 1), opnd{128});
		E.sop1(S1_SWAPPC_B64, S_LINK, sreg(S_LINK));
	}
	// A packet load whose bytes were loaded ahead into VGPR `tmp` (general kernels, see
	// asm_cc.cpp plan_hoists): the bounds check at its own place (MEM fault for lanes whose
	// packet is shorter than off + z, like the handler), then wait for it (vmcnt <= the loads
	// issued after it) and copy.
	//
	// With the run mask (s[76:77], see asm_cc.cpp) the lanes in the mask hold the load already
	// and cannot fault on it; only when a running lane is outside the mask does the use compare:
	// fault the lanes past their packet's end, load for the others directly (and wait for it).
	void ldx_hoisted(int d, int z, uint32_t off, int tmp, uint32_t later, uint32_t fault_off,
			 bool runmask)
	{
		size_t over = 0;
		if (runmask) {
			E.sop2(S2_ANDN2_B64, S_MASK, opnd{SRC_EXEC}, sreg(AH_S_RUNMASK));
			over = E.fwd(SP_CBRANCH_SCC0); // over the block below
		}
		fault_past(off + (uint32_t)z, fault_off);
		if (runmask) {
			E.sop2(S2_ANDN2_B64, S_MASK, opnd{SRC_EXEC}, sreg(AH_S_RUNMASK)); // in bounds, unmasked
			E.sopp(SP_CBRANCH_SCC0, 6);                                      // over the 6 dwords below
			E.sop1(S1_MOV_B64, S_JUNK, opnd{SRC_EXEC});
			E.sop1(S1_MOV_B64, SRC_EXEC, sreg(S_MASK));
			E.global_load(__builtin_ctz(z), tmp, V_PKT, off);
			E.wait_vm(0);
			E.sop1(S1_MOV_B64, SRC_EXEC, sreg(S_JUNK));
			E.to(over);
		}
		E.wait_vm(later);
		E.vop1(z == 8 ? V1_MOV_B64 : V1_MOV_B32, L(d), vreg(tmp));
		loaded(d, z);
	}
	// FAULT entry (structured): fault every running lane with `code`
	void fault(uint32_t code, uint32_t fault_off)
	{
		E.sop1(S1_MOV_B32, S_CODE, k32(code));
		E.sop1(S1_MOV_B64, S_MASK, opnd{SRC_EXEC});
		call_routine(fault_off, 0);
	}

	// ---- conditional jumps: VCC = lanes taking the branch (the caller appends the tail)
	// c: the condition, AH_CC_* (the generator's CONDS)
	static bool eval(int c, uint64_t a, uint64_t b)
	{
		const int64_t sa = (int64_t)a, sb = (int64_t)b;
		switch (c) {
		case AH_CC_JEQ: return a == b;
		case AH_CC_JNE: return a != b;
		case AH_CC_JGT: return a > b;
		case AH_CC_JGE: return a >= b;
		case AH_CC_JLT: return a < b;
		case AH_CC_JLE: return a <= b;
		case AH_CC_JSGT: return sa > sb;
		case AH_CC_JSGE: return sa >= sb;
		case AH_CC_JSLT: return sa < sb;
		case AH_CC_JSLE: return sa <= sb;
		default: return (a & b) != 0; // AH_CC_JSET
		}
	}
	static bool is_signed(int c)
	{
		return c == AH_CC_JSGT || c == AH_CC_JSGE || c == AH_CC_JSLT || c == AH_CC_JSLE;
	}
	// the VOPC predicate of a condition other than JSET (signedness is the opcode base's)
	static int pred(int c)
	{
		switch (c) {
		case AH_CC_JEQ: return P_EQ;
		case AH_CC_JNE: return P_NE;
		case AH_CC_JGT: case AH_CC_JSGT: return P_GT;
		case AH_CC_JGE: case AH_CC_JSGE: return P_GE;
		case AH_CC_JLT: case AH_CC_JSLT: return P_LT;
		default: return P_LE; // AH_CC_JLE, AH_CC_JSLE
		}
	}
	static int swapped(int p)
	{
		switch (p) {
		case P_GT: return P_LT;
		case P_GE: return P_LE;
		case P_LT: return P_GT;
		case P_LE: return P_GE;
		default: return p;
		}
	}
	// a compare decided at compile time: no code, the layout falls through or jumps
	bool taken_sets_vcc = false; // structured programs (and CC_OFF_STATIC_TAKEN)
	void decided(bool taken)
	{
		if (taken_sets_vcc && taken) { // structured: s_mov_b64 vcc, exec (the split sends every lane)
			E.sop1(S1_MOV_B64, SRC_VCC, opnd{SRC_EXEC});
			return;
		}
		// (structured and never taken: the code generator only empties the join mask)
		blk.sdir = taken ? 1 : 0;
	}
	void cond_imm(int c, int d, uint64_t K)
	{
		const rf &x = f.r[d];
		if (x.c) {
			decided(eval(c, x.v, K));
			return;
		}
		if (K == 0 && x.nz && (c == AH_CC_JEQ || c == AH_CC_JNE)) { // NULL check of a lookup that cannot fail
			decided(c == AH_CC_JNE);
			return;
		}
		use(d);
		if (c == AH_CC_JSET) {
			const uint32_t lo = (uint32_t)K, hi = hz(d) ? 0u : (uint32_t)(K >> 32);
			if (!lo && !hi) {
				decided(false);
				return;
			}
			if (!hi) {
				E.vop2(V2_AND, T0, k32(lo), L(d));
				E.vopc(VC_U32 + P_NE, opnd{128}, T0);
			} else {
				E.vop2(V2_AND, T0, k32(lo), L(d));
				E.vop2(V2_AND, T1, k32(hi), Hi(d));
				E.vopc(VC_U64 + P_NE, opnd{128}, T0);
			}
			return;
		}
		if (hz(d)) {
			// d in [0, 2^32): K outside that range decides statically, and the same way for every
			// such d (unsigned: K is above all of them; signed: on one side of all of them)
			if (K >> 32) {
				decided(eval(c, 0, K));
				return;
			}
			E.vopc(VC_U32 + swapped(pred(c)), k32((uint32_t)K), L(d));
			return;
		}
		E.vopc((is_signed(c) ? VC_I64 : VC_U64) + swapped(pred(c)), opnd{c64(K)}, L(d));
	}
	void cond_reg(int c, int d, int s)
	{
		if (f.r[s].c) {
			cond_imm(c, d, f.r[s].v);
			return;
		}
		use(d);
		use(s);
		if (c == AH_CC_JSET) {
			E.vop2(V2_AND, T0, vreg(L(s)), L(d));
			if (hz(d) || hz(s)) {
				E.vopc(VC_U32 + P_NE, opnd{128}, T0);
			} else {
				E.vop2(V2_AND, T1, vreg(Hi(s)), Hi(d));
				E.vopc(VC_U64 + P_NE, opnd{128}, T0);
			}
			return;
		}
		if (hz(d) && hz(s)) {
			E.vopc(VC_U32 + pred(c), vreg(L(d)), L(s));
			return;
		}
		E.vopc((is_signed(c) ? VC_I64 : VC_U64) + pred(c), vreg(L(d)), L(s));
	}
	// JMP32: compares of the low words (sign-extended, they compare alike under every condition)
	static bool eval32(int c, uint32_t a, uint32_t b)
	{
		return eval(c, (uint64_t)(int64_t)(int32_t)a, (uint64_t)(int64_t)(int32_t)b);
	}
	void cond32_imm(int c, int d, uint32_t K)
	{
		const rf &x = f.r[d];
		if (x.c) {
			decided(eval32(c, (uint32_t)x.v, K));
			return;
		}
		use(d);
		if (c == AH_CC_JSET) {
			if (!K) {
				decided(false);
				return;
			}
			E.vop2(V2_AND, T0, k32(K), L(d));
			E.vopc(VC_U32 + P_NE, opnd{128}, T0);
			return;
		}
		E.vopc((is_signed(c) ? VC_I32 : VC_U32) + swapped(pred(c)), k32(K), L(d));
	}
	void cond32_reg(int c, int d, int s)
	{
		if (f.r[s].c) {
			cond32_imm(c, d, (uint32_t)f.r[s].v);
			return;
		}
		use(d);
		use(s);
		if (c == AH_CC_JSET) {
			E.vop2(V2_AND, T0, vreg(L(s)), L(d));
			E.vopc(VC_U32 + P_NE, opnd{128}, T0);
			return;
		}
		E.vopc((is_signed(c) ? VC_I32 : VC_U32) + pred(c), vreg(L(d)), L(s));
	}
};

} // namespace
