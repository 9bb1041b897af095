// asm_cc.cpp — optimising gfx950 code generation for compiled programs (variant 0).
//
// asm_jit.cpp lays a lowered program (asm_lower) out as straight-line code; for each entry it
// can copy the interpreter's handler body verbatim.  Handler bodies are written for any register
// contents, so they pay for 64-bit generality everywhere: a 32-bit result re-zeroes its high
// half, a 64-bit multiply by a 32-bit constant multiplies by a zero high word, a compare of a
// loaded byte is a 64-bit compare against an SGPR pair set by two scalar moves, a map lookup
// re-reads its key from the stack and re-checks the result's range at every use.
//
// Here two forward passes and one backward pass over the state tree (the translator gives every
// entry one predecessor, so facts are exact per path) compile the hot families to hand-encoded
// gfx950 instructions instead:
//   facts (forward): per eBPF register, a known constant, the number of known leading zero bits,
//     non-NULL-ness, and for a map lookup result the map and the register holding its index;
//     per stack word, the register whose low bytes it holds (store-to-load forwarding);
//     compares against constants refine the facts on their taken / fall-through edges;
//   liveness (backward): pure operations (ALU, byte swaps, staged packet and stack loads,
//     lookups with a statically resolved map) whose result no path reads emit nothing, and the
//     group's register zeroing covers only the registers the program reads before writing;
//   emission (forward):
//   * constants fold (both operands known: a move of the result);
//   * high halves known zero are neither recomputed nor re-zeroed;
//   * 64-bit AND/OR/XOR/shift by constants become 32-bit operations where a half is unchanged
//     or zero, shifts by >= 32 become moves;
//   * MUL by a constant drops the partial products of known-zero words, multiplies by powers
//     of two become shifts;
//   * compares of values below 2^32 against constants below 2^32 are single VOPC e32
//     instructions with the constant as a literal; statically decided compares (including
//     NULL checks of lookups that cannot fail) become VCC = EXEC or 0;
//   * a staged packet load followed by BE16/BE32 of the same register is one v_perm_b32 that
//     picks the bytes in network order straight from the staged packet registers;
//   * stack stores/loads at known offsets are single LDS instructions with the offset folded in;
//     a load of a word stored from a register that is unchanged since reads the register;
//   * an array-map lookup whose key comes from a register proven below max_entries cannot
//     return NULL: r0 = base + key * value_size (one v_mad_u64_u32, or nothing if r0 is only
//     dereferenced), and loads through it read the workgroup's LDS copy of the map at
//     lds_off + key * value_size + off with no range check.
// Everything else (memory through unknown pointers, generic lookups, division, generic exits,
// faults) still copies the interpreter's handler body, so semantics there are unchanged.
//
// Files: asm_cc_facts.h (registers, facts, the family table), asm_cc_emit.h (per-entry emission),
// this file (the passes: cc_compile); the machine words are encoded by gfx950_enc.h, which
// asm_jit.cpp shares.
#include "asm_cc_emit.h"

namespace {

// ---------------------------------------------------------------- driver
// General kernels: packet loads at constant offsets (LDXPKTG, one memory round trip each) are
// issued ahead at the head of the straight run that contains them, into the image's spare
// VGPRs, so their latencies overlap (plan_hoists).  Indexed by entry.
struct hoist_plan {
	std::vector<int16_t> tmp;               // >= 0: the entry's load arrives in this VGPR (pair)
	std::vector<uint16_t> later;            // loads issued after it that may still be in flight
	std::vector<std::vector<uint32_t>> at;  // run head: the loads to issue there
	std::vector<uint32_t> next;             // the load to issue after this one is used
	std::vector<uint32_t> run_ext;          // run head: the largest off + size of its hoisted loads
};

// one lowered entry, decoded
struct entry {
	size_t k;        // its place in the layout order
	uint32_t e, h;   // entry index, handler id
	int fam, cls, d, s;
	uint64_t K;      // the immediate
	uint32_t aux0, aux1;
};

// What the passes of one compilation share.  Two forward passes and a backward pass in between
// (cc_compile): the first forward pass computes facts and records what each entry reads and
// writes, liveness turns that into live_out / live_start, and the final forward pass emits.
struct compiler {
	// inputs
	const dprog_host &xl;
	const std::vector<dp_entry> &low;
	const std::vector<uint32_t> &order;
	const std::vector<char> &entry_point;
	const int mode;
	const bool structured;
	const cc_routines &rt;
	const std::vector<dp_map> &table;
	const cc_options &opt;
	std::vector<cc_block> &out;
	const size_t n;
	std::vector<mapinfo> maps;
	// Run mask (general kernels: s[76:77]): the run head tests every running lane against the
	// run's largest load extent once (one VALU compare into s[76:77]); the run's loads are issued
	// for those lanes with no per-load compare, and a use only compares (bounds check, fault,
	// direct load) when some running lane missed the mask.  Two VALU per hoisted load fewer.
	const bool runmask;
	// general kernels (parking scheduler, no join SGPRs): s[74:75] is free for the short-lane
	// mask of the inline header loads (ldxpkc_general)
	const bool gen_short_mask;
	bool uses_short_mask = false;
	std::vector<uint32_t> npred; // predecessors (the tree gives one; shared fault entries get no facts)
	hoist_plan hoist;
	// the first forward pass's record of each entry, and the liveness computed from it
	std::vector<uint16_t> uses, live_out;
	std::vector<int8_t> defreg;
	std::vector<char> pure;
	uint16_t live_start = 0x7ff;
	// state of one forward pass
	std::vector<facts> in;
	std::vector<char> have;
	std::vector<char> fused;           // a BSWAP folded into the preceding packet load
	std::vector<int8_t> movfuse_src;   // this entry reads a fused MOV's source
	std::vector<int16_t> movfuse_fam;  // ... as this 32-bit operation

	compiler(const dprog_host &x, const std::vector<dp_entry> &l, const std::vector<uint32_t> &o,
		 const std::vector<char> &ep, int m, bool st, const cc_routines &r,
		 const std::vector<dp_map> &t, const cc_options &op, std::vector<cc_block> &ou)
	    : xl(x), low(l), order(o), entry_point(ep), mode(m), structured(st), rt(r), table(t), opt(op),
	      out(ou), n(l.size()), runmask(m == 0 && op.runmask),
	      gen_short_mask(m == 0 && !st && !AH_GEN_JOIN && op.short_mask), npred(n, 0), uses(n, 0),
	      live_out(n, 0xffff), defreg(n, -1), pure(n, 0)
	{
		for (const dp_map &mp : table)
			maps.push_back(mapinfo{mp.dev_base, mp.value_size, mp.max_entries, mp.lds_off});
	}

	int fam_of(uint32_t e) const { return ah_fam[(uint32_t)low[e].handler]; }
	bool is_cond(uint32_t e) const { return (ah_flags[(uint32_t)low[e].handler] & 1) != 0; }
	bool is_leaf(uint32_t e) const { return fam_of(e) == AHF_EXIT || fam_of(e) == AHF_FAULT; }

	entry decode(size_t k) const
	{
		entry x;
		x.k = k;
		x.e = order[k];
		x.h = (uint32_t)low[x.e].handler;
		x.fam = ah_fam[x.h];
		x.cls = class_of(x.fam);
		x.d = ah_dst[x.h];
		x.s = ah_src[x.h];
		x.K = low[x.e].imm;
		memcpy(&x.aux0, reinterpret_cast<const uint8_t *>(&low[x.e]) + AH_E_AUX0, 4);
		memcpy(&x.aux1, reinterpret_cast<const uint8_t *>(&low[x.e]) + AH_E_AUX1, 4);
		return x;
	}

	void count_predecessors()
	{
		for (uint32_t e : order) {
			if (is_leaf(e))
				continue;
			if (xl.entries[e].next < n)
				npred[xl.entries[e].next]++;
			if (is_cond(e) && xl.entries[e].target < n)
				npred[xl.entries[e].target]++;
		}
	}

	// the entry after order[k] if control reaches it only by falling through from order[k]
	// (UINT32_MAX: none): an operation there can be fused into this one
	uint32_t sole_successor(size_t k) const
	{
		const uint32_t nx = xl.entries[order[k]].next;
		if (nx < n && k + 1 < order.size() && order[k + 1] == nx && !entry_point[nx] && npred[nx] == 1)
			return nx;
		return UINT32_MAX;
	}

	// A run ends at an entry point, a branch, a non-fall-through successor, a store that may hit
	// the packet or a scheduler hand-off.
	void plan_hoists()
	{
		hoist.tmp.assign(n, -1);
		hoist.later.assign(n, 0);
		hoist.at.assign(n, std::vector<uint32_t>());
		hoist.next.assign(n, UINT32_MAX);
		hoist.run_ext.assign(n, 0);
		const int hoist_regs = AH_GEN_HOIST_REGS;
		const int slot_regs = 2;
		if (mode != 0 || hoist_regs <= 0 || !opt.hoist)
			return;
		auto breaks_after = [&](uint32_t e) {
			// (letting runs continue past conditionals along the fall-through edge, loads
			// issued for lanes that branch away, measured 3% slower on C5)
			return is_cond(e) || is_leaf(e) || fam_of(e) == AHF_LOOKUPGEN ||
			       is_store_through_pointer(class_of(fam_of(e)));
		};
		for (size_t k = 0, j; k < order.size(); k = j + 1) {
			j = k; // run [k, j]
			while (j + 1 < order.size() && !breaks_after(order[j]) &&
			       xl.entries[order[j]].next == order[j + 1] && !entry_point[order[j + 1]])
				j++;
			// the run's loads, issued through a ring of 2-VGPR slots: the first `slots` at the
			// run head, load i + slots right after load i is consumed (its slot is free again)
			std::vector<uint32_t> ld;
			for (size_t q = k; q <= j; q++) {
				const uint32_t e = order[q];
				if (class_of(fam_of(e)) == AHC_LDXPKTG &&
				    low[e].imm + (uint64_t)size_of(fam_of(e)) <= 4095u)
					ld.push_back(e);
			}
			if (ld.size() < 2)
				continue;
			const uint32_t head = order[k];
			const size_t slots = (size_t)(hoist_regs / slot_regs);
			size_t issued = std::min(slots, ld.size());
			hoist.at[head].assign(ld.begin(), ld.begin() + issued);
			for (uint32_t x : ld)
				hoist.run_ext[head] = std::max<uint32_t>(hoist.run_ext[head],
									 (uint32_t)low[x].imm + (uint32_t)size_of(fam_of(x)));
			for (size_t i = 0; i < ld.size(); i++) {
				hoist.tmp[ld[i]] = (int16_t)(AH_GEN_HOIST_BASE + slot_regs * (i % slots));
				hoist.later[ld[i]] = (uint16_t)(issued - 1 - i);
				if (i + slots < ld.size()) {
					hoist.next[ld[i]] = ld[i + slots];
					issued++;
				}
			}
		}
	}

	// issue packet load x into its ring slot, for the lanes whose packet holds it
	// (masked: exec is already the lanes to load for, the run head's batch)
	void issue(enc &Hq, uint32_t x, bool masked = false) const
	{
		const int fx = fam_of(x);
		const uint32_t K32 = (uint32_t)low[x].imm;
		if (masked) {
		} else if (runmask) {
			Hq.sop1(S1_AND_SAVEEXEC_B64, S_JUNK, sreg(AH_S_RUNMASK));
		} else {
			Hq.vopc(VC_U32 + P_LE, k32(K32 + (uint32_t)size_of(fx)), V_LEN); // vcc = off+z <= len
			Hq.sop1(S1_AND_SAVEEXEC_B64, S_JUNK, opnd{SRC_VCC});
		}
		Hq.global_load(ah_fam_idx[fx], hoist.tmp[x], V_PKT, K32);
		if (!masked)
			Hq.sop1(S1_MOV_B64, SRC_EXEC, sreg(S_JUNK));
	}

	// the head of a run of hoisted loads: its first loads, issued before anything else of the block
	void emit_run_head(uint32_t e, cc_block &blk) const
	{
		if (hoist.at[e].empty())
			return;
		enc Hq{blk.hoist};
		if (runmask) { // s[76:77] = the running lanes whose packet holds every load of the run
			Hq.vopc(VC_U32 + P_LE, k32(hoist.run_ext[e]), V_LEN); // vcc = ext <= len (v40)
			Hq.sop1(S1_MOV_B64, AH_S_RUNMASK, opnd{SRC_VCC});
			Hq.sop1(S1_AND_SAVEEXEC_B64, S_JUNK, opnd{SRC_VCC});  // s[60:61] = exec
			for (uint32_t x : hoist.at[e])
				issue(Hq, x, true);
			Hq.sop1(S1_MOV_B64, SRC_EXEC, sreg(S_JUNK));
		} else {
			for (uint32_t x : hoist.at[e])
				issue(Hq, x);
		}
	}

	// A 32-bit MOV d = s whose only successor operates on d with an immediate: the successor
	// reads s directly and the MOV emits nothing (one VALU move saved).  True: fused, the
	// successor is told (movfuse_*).
	bool fuse_mov(const entry &x, emitter &em)
	{
		if (x.fam != AHF_A32R_MOV || x.d == x.s || x.d >= AH_NREGS || x.s >= AH_NREGS || (opt.off & CC_OFF_DEAD))
			return false;
		const uint32_t nx = sole_successor(x.k);
		if (nx == UINT32_MAX || hoist.tmp[nx] >= 0)
			return false;
		const uint32_t h2 = (uint32_t)low[nx].handler;
		const uint32_t K2 = (uint32_t)low[nx].imm;
		if (ah_dst[h2] != x.d)
			return false;
		int as32 = -1;
		switch (ah_fam[h2]) {
		case AHF_A32I_ADD: case AHF_A32I_SUB: case AHF_A32I_OR: case AHF_A32I_AND: case AHF_A32I_XOR:
		case AHF_A32I_LSH: case AHF_A32I_RSH:
			as32 = ah_fam[h2]; // (see alu32i)
			break;
		case AHF_A64I_RSH:
			if (K2 < 32)
				as32 = AHF_A32I_RSH; // (u32 >> c)
			break;
		case AHF_A64I_LSH:
			if (K2 < 32 && std::min(32, bits_of(em.f.r[x.s])) + (int)K2 <= 32)
				as32 = AHF_A32I_LSH; // (the result still fits 32 bits)
			break;
		default:
			break;
		}
		if (as32 < 0)
			return false;
		movfuse_src[nx] = (int8_t)x.s;
		movfuse_fam[nx] = (int16_t)as32;
		em.use(x.s);
		return true;
	}

	// a staged packet load of at most 4 bytes followed by BE16 / BE32 of its destination: the
	// load swaps (returns the swap's bytes, 0: none) and the BSWAP emits nothing
	int fuse_bswap(const entry &x)
	{
		const uint32_t nx = sole_successor(x.k);
		if (mode != 1 || size_of(x.fam) > 4 || nx == UINT32_MAX)
			return 0;
		const uint32_t h2 = (uint32_t)low[nx].handler;
		const int f2 = ah_fam[h2];
		if ((f2 != AHF_BSWAP16 && f2 != AHF_BSWAP32) || ah_dst[h2] != x.d)
			return 0;
		fused[nx] = 1;
		return f2 == AHF_BSWAP16 ? 2 : 4;
	}

	// HLOOKUP: the generic routine, whose probe of a key of <= 8 bytes also loads the slot's first
	// 8 value bytes (AH_V_HVAL, the kernels' .Lr_hlookup): they are kept in a register D dead from
	// here on, so that loads through the result (LDXHV) become register extracts (one memory
	// round trip less).
	// (an inline jhash + home-slot probe, round 3, measured 3% slower than the generic routine on
	// C4H and was retired in round 5)
	bool emit_hlookup(const entry &x, emitter &em, bool final_pass)
	{
		facts &f = em.f;
		const int mi = (int)(x.aux0 / sizeof(dp_map));
		if (!final_pass || mi >= (int)table.size() || !(table[mi].flags & DP_MAP_HASH) ||
		    dp_hash_key_size(table[mi].flags) > 8 || !opt.hash_forward)
			return false;
		// D must also be free of every fact that reads its VGPRs through another name
		// (a stack word forwarded from D, a map pointer indexed by D): dropping such a
		// fact here, where the pass that computed liveness kept it, changes the facts
		// downstream (a load forwarded there, a constant exit, dead code removed for
		// it) — found by the hashtable fuzz mode
		auto aliased = [&](int r) {
			for (uint8_t i = 0; i < f.nst; i++)
				if (f.st[i].reg == r)
					return true;
			for (int q = 0; q < AH_NREGS; q++)
				if (f.r[q].mreg == r)
					return true;
			return false;
		};
		int D = -1;
		for (int r = 9; r >= 2 && D < 0; r--)
			if (!(live_out[x.e] & (1u << r)) && !aliased(r))
				D = r;
		if (D < 0)
			return false;
		em.blk.reads |= (uint8_t)(1u << 4); // s14 = the map record offset
		em.blk.sval[4] = x.aux0;
		em.use(2);
		em.call_routine(rt.hlookup, 0);
		em.E.vop1(V1_MOV_B64, 2 * D, vreg(AH_V_HVAL));
		f.def(0, rf());
		// (D's value facts stay: the liveness that picked D was computed with
		// them, so a compare they decided must stay decided — dropping them
		// made such a compare read D's VGPRs, now the forwarded value; with D
		// unaliased, clobber_phys drops nothing else)
		f.clobber_phys(D);
		f.r[0].hfwd = (int8_t)D;
		f.t2zero = false;
		return true;
	}

	// Emit entry x's family as compiled code.  False: the family (or this instance of it) has no
	// compiled form, the caller copies the interpreter's handler body.  *spec_map: a map load
	// compiled against the LDS copy (pure, unlike the generic one).
	bool emit_family(const entry &x, emitter &em, bool final_pass, bool *spec_map)
	{
		facts &f = em.f;
		const int d = x.d, s = x.s;
		const uint64_t K = x.K;
		switch (x.cls) {
		case AHC_NOP:
			return true;
		case AHC_EXIT:
			if (f.r[0].c && !(opt.off & CC_OFF_EXIT_KNOWN))
				em.exit_known(f.r[0].v, rt.exit_k, structured);
			else if (structured && !opt.exit_call)
				em.exit_inline();
			else if (structured)
				em.call_routine(rt.exit, 1);
			else
				return false;
			return true;
		case AHC_FAULT:
			if (!structured)
				return false;
			em.fault(x.aux0, rt.fault);
			return true;
		case AHC_A64I:
			switch (x.fam) {
			case AHF_A64I_MOV: em.mov64(d, K); return true;
			case AHF_A64I_ADD: em.add64i(d, K); return true;
			case AHF_A64I_OR: em.or64i(d, K); return true;
			case AHF_A64I_XOR: em.xor64i(d, K); return true;
			case AHF_A64I_AND: em.and64i(d, K); return true;
			case AHF_A64I_LSH: em.lsh64i(d, (uint32_t)K); return true;
			case AHF_A64I_RSH: em.rsh64i(d, (uint32_t)K); return true;
			case AHF_A64I_MUL: em.mul64i(d, K); return true;
			default: return false; // (DIV, MOD)
			}
		case AHC_A32I: return em.alu32i(x.fam, d, (uint32_t)K);
		case AHC_A32R: return em.alu32r(x.fam, d, s);
		case AHC_A64R: return em.alu64r(x.fam, d, s);
		case AHC_JI: em.cond_imm(cond_of(x.fam), d, K); return true;
		case AHC_JR: em.cond_reg(cond_of(x.fam), d, s); return true;
		case AHC_J32I: em.cond32_imm(cond_of(x.fam), d, (uint32_t)K); return true;
		case AHC_J32R: em.cond32_reg(cond_of(x.fam), d, s); return true;
		case AHC_MOV64R: em.copy64(d, s); return true;
		case AHC_BSWAP:
			if (fused[x.e]) {
				em.use(d); // the value the fused load produced
				return true;
			}
			return em.bswap(x.fam, d);
		case AHC_LDXPKC: {
			const int z = size_of(x.fam);
			if (mode == 0) { // general kernels: length checks against the short-lane mask
				if (!gen_short_mask || s + z > 64)
					return false;
				em.ldxpkc_general(d, z, s, rt.fault);
				uses_short_mask = true;
				return true;
			}
			em.ldxpkc(d, z, s, fuse_bswap(x));
			return true;
		}
		case AHC_LDXPKTV: {
			const int z = size_of(x.fam);
			const int64_t Ks = (int64_t)K;
			if (mode != 1 || Ks < 0 || Ks > 64 - z || d >= AH_NREGS || s >= AH_NREGS || !opt.pktv)
				return false;
			em.ldxpktv_staged(d, s, z, (uint32_t)Ks, (int)x.h);
			em.used |= copied_uses(x.fam, d, s); // (the spliced slow path's reads)
			return true;
		}
		case AHC_STXSTK:
			if (K + 8 > 255 * 4)
				return false;
			em.stxstk(size_of(x.fam), d, (uint32_t)K);
			return true;
		case AHC_LDXSTK:
			if (K + 8 > 255 * 4)
				return false;
			em.ldxstk(size_of(x.fam), d, (uint32_t)K);
			return true;
		case AHC_LOOKUPSTK: {
			int mi = -1;
			for (size_t t = 0; t < maps.size(); t++)
				if (maps[t].dev_base == K && maps[t].max_entries == low[x.e].target &&
				    maps[t].value_size == x.aux1)
					mi = (int)t;
			return !(opt.off & CC_OFF_LOOKUP) && em.lookup_stk(mi, x.aux0);
		}
		case AHC_LDXMAP:
			return *spec_map = em.ldxmap(size_of(x.fam), d, s, K);
		case AHC_HLOOKUP:
			return emit_hlookup(x, em, final_pass);
		case AHC_LDXHV:
			return em.ldxhv_fwd(size_of(x.fam), d, s, (int32_t)x.aux0);
		default:
			return false;
		}
	}

	// the interpreter's body instead of compiled code; the facts of what it writes are lost
	void copied_body(const entry &x, emitter &em, const facts &before, int wr)
	{
		facts &f = em.f;
		f = before;
		f.t2zero = false; // (handler bodies use v46..v51 freely)
		em.blk.fast = false;
		em.blk.body.clear();
		em.blk.splice_h = -1;
		em.blk.reads = 0;
		em.used = copied_uses(x.fam, x.d, x.s);
		if (wr >= 0)
			f.def(wr, copied_result(x.fam));
		// stores through unknown pointers may hit the stack
		if (is_store_through_pointer(x.cls))
			f.nst = 0;
		if (x.cls == AHC_STSTK)
			f.store(x.aux0, size_of(x.fam), -1);
	}

	// hand the facts after entry x to its successors (a compare against a constant refines them
	// on its two edges)
	void give_successors(const entry &x, const facts &f)
	{
		if (is_leaf(x.e))
			return;
		auto give = [&](uint32_t to, const facts &fo) {
			if (to >= n)
				return;
			in[to] = fo;
			have[to] = 1;
		};
		const uint32_t nx = xl.entries[x.e].next;
		if (!is_cond(x.e)) {
			give(nx, f);
			return;
		}
		facts ft = f, fn = f;
		// (JMP32 edges refine nothing)
		if ((x.cls == AHC_JI || (x.cls == AHC_JR && f.r[x.s].c)) && x.d < AH_NREGS) {
			const uint64_t cv = x.cls == AHC_JI ? x.K : f.r[x.s].v;
			refine(ft, cond_of(x.fam), x.d, cv, true);
			refine(fn, cond_of(x.fam), x.d, cv, false);
		}
		give(xl.entries[x.e].target, ft);
		give(nx, fn);
	}

	// One pass over the entries in layout order (parents before children, so each entry's facts
	// are there when it is reached).  The first pass records uses / defreg / pure for liveness;
	// the final one, which has live_out and live_start, drops what is dead and picks the dead
	// register of a hashtable probe (emit_hlookup), and its code is the result.
	void forward_pass(bool final_pass)
	{
		out.assign(n, cc_block());
		in.assign(n, facts());
		have.assign(n, 0);
		fused.assign(n, 0);
		movfuse_src.assign(n, -1);
		movfuse_fam.assign(n, -1);
		if (xl.start < n) {
			facts f0; // r0, r2..r9 are zero at the start (the kernel, or the prologue below)
			for (int r = 0; r < AH_NREGS; r++) {
				f0.r[r] = (r == 1 || r == 10) ? rf() : kconst(0);
				f0.pv[r] = (live_start & (1u << r)) != 0;
			}
			in[xl.start] = f0;
			have[xl.start] = 1;
		}
		for (size_t k = 0; k < order.size(); k++) {
			const entry x = decode(k);
			const uint32_t e = x.e;
			const bool valid = have[e] && npred[e] == (e == xl.start ? 0u : 1u);
			facts f = valid ? in[e] : facts();
			if (!valid)
				for (bool &p : f.pv)
					p = true;
			cc_block &blk = out[e];
			f.nofwd = (opt.off & CC_OFF_STACK_FWD) != 0;
			const facts before = f;
			emitter em(blk, f, maps);
			em.taken_sets_vcc = structured || (opt.off & CC_OFF_STATIC_TAKEN); // compares leave VCC
			emit_run_head(e, blk);
			bool ok = true, spec_map = false;
			if (fuse_mov(x, em)) {
				// (nothing emitted; d keeps its old facts until the fused operation defines it)
			} else if (movfuse_src[e] >= 0) {
				ok = em.alu32i(movfuse_fam[e], x.d, (uint32_t)x.K, movfuse_src[e]);
			} else if (hoist.tmp[e] >= 0) {
				em.ldx_hoisted(x.d, size_of(x.fam), (uint32_t)x.K, hoist.tmp[e], hoist.later[e], rt.fault,
					       runmask);
				if (hoist.next[e] != UINT32_MAX)
					issue(em.E, hoist.next[e]);
			} else {
				ok = emit_family(x, em, final_pass, &spec_map);
			}
			const int wr = written_reg(x.fam, x.d);
			if (ok)
				blk.fast = true;
			else
				copied_body(x, em, before, wr);
			if (!final_pass) {
				uses[e] = em.used;
				defreg[e] = (int8_t)wr;
				pure[e] = (char)(pure_fam(x.fam, spec_map) && wr >= 0 &&
						 !(mode == 0 && x.cls == AHC_LDXPKC));
			} else if (!(opt.off & CC_OFF_DEAD) && pure[e] && wr >= 0 && !(live_out[e] & (1u << wr))) {
				// dead: no code, the register's VGPRs do not hold the (unused) value
				blk.fast = true;
				blk.body.clear();
				blk.splice_h = -1;
				blk.reads = 0;
				f.pv[wr] = false;
				f.t2zero = before.t2zero; // (its code, which may have zeroed v48, is gone)
			}
			give_successors(x, f);
		}
	}

	// liveness (backward over the tree: children come after their parent in `order`)
	void liveness()
	{
		std::vector<uint16_t> live_in(n, 0);
		for (size_t k = order.size(); k-- > 0;) {
			const uint32_t e = order[k];
			uint16_t lo = 0;
			if (!is_leaf(e)) {
				const uint32_t nx = xl.entries[e].next;
				if (nx < n)
					lo |= npred[nx] == 1 ? live_in[nx] : 0x7ff;
				if (is_cond(e) && xl.entries[e].target < n) {
					const uint32_t tk = xl.entries[e].target;
					lo |= npred[tk] == 1 ? live_in[tk] : 0x7ff;
				}
			}
			live_out[e] = lo;
			uint16_t li = lo;
			if (defreg[e] >= 0 && !(uses[e] & (1u << defreg[e])))
				li &= (uint16_t)~(1u << defreg[e]);
			if (pure[e] && defreg[e] >= 0 && !(lo & (1u << defreg[e])))
				li = lo; // a dead pure operation reads nothing
			else
				li |= uses[e];
			live_in[e] = li;
		}
		live_start = xl.start < n ? live_in[xl.start] : 0x7ff;
		if (opt.off & (CC_OFF_DEAD | CC_OFF_ZERO_ALL))
			live_start = 0x7ff;
	}

	// does anything read the packet address (staged mode: the prologue computes it only then)?
	// The generic memory routines and r1 do.
	bool needs_packet_address() const
	{
		if (live_start & (1u << 1))
			return true;
		for (uint32_t e : order) {
			const int cls = class_of(fam_of(e));
			if (!out[e].fast && (cls == AHC_LDXGEN || cls == AHC_LDXPKTG || cls == AHC_LOOKUPGEN ||
					     cls == AHC_UPDATE || cls == AHC_HDELETE || is_store_through_pointer(cls)))
				return true;
			// (compiled LDXPKTV reads the packet address too, and so does its spliced slow path)
			if (cls == AHC_LDXPKTV)
				return true;
		}
		return false;
	}

	// Dead stack stores: when no code of the program can read its stack frame — every
	// block is one of the families below, stack loads all forwarded from registers,
	// lookups compiled with their key in a register — the stores into the frame are
	// never observed, and emit nothing (C4: the key STXW, one LDS write per packet).
	// Anything that may read the frame (generic or run-time-offset loads, the lookup,
	// update and delete routines, hashtable probes, counters through pointers, a
	// copied handler body of a load or a lookup) keeps every store.
	void drop_dead_stack_stores()
	{
		if (!opt.drop_stores)
			return;
		for (uint32_t e : order) {
			switch (class_of(fam_of(e))) {
			case AHC_A64R: case AHC_A32R: case AHC_JR: case AHC_A64I: case AHC_A32I: case AHC_BSWAP:
			case AHC_JI: case AHC_MOV64R: case AHC_NEG64: case AHC_NEG32: case AHC_ARSH64I:
			case AHC_ARSH64R: case AHC_ARSH32I: case AHC_ARSH32R: case AHC_DIV64Z: case AHC_MOD64Z:
			case AHC_DIV32Z: case AHC_MOD32Z: case AHC_J32R: case AHC_J32I: case AHC_STXSTK:
			case AHC_STSTK: case AHC_LDXPKTG: case AHC_LDXPKC: case AHC_LDXPKBE: case AHC_EXIT:
			case AHC_FAULT: case AHC_NOP: case AHC_LOOPINIT: case AHC_LOOPCNT: case AHC_OVLINIT:
				break; // never reads the frame, compiled or copied
			case AHC_LDXMAP: case AHC_LDXSTK: case AHC_LOOKUPSTK:
				if (!out[e].fast || out[e].stack_read)
					return;
				break;
			default:
				return;
			}
		}
		for (uint32_t e : order) {
			const int cls = class_of(fam_of(e));
			if (cls == AHC_STXSTK || cls == AHC_STSTK) {
				out[e].fast = true;
				out[e].body.clear();
				out[e].splice_h = -1;
				out[e].reads = 0;
			}
		}
	}

	// the group set-up the kernel leaves to compiled programs (cc_prologue), in the start block
	void emit_prologue(bool needs_pkt)
	{
		if (xl.start >= n)
			return;
		cc_prologue(mode, live_start, needs_pkt, structured, out[xl.start].prologue);
		if (uses_short_mask) { // s[74:75] = lanes whose packet is shorter than 64 B
			enc P{out[xl.start].prologue};
			P.vop3(VC_U32 + P_GT, S_SHORT, 128 + 64, VGPR0 + V_LEN, 0);
		}
	}
};

} // namespace

// (each name's meaning: asm_cc.h cc_options)
cc_options
cc_read_options()
{
	auto set = [](const char *name) { return getenv(name) != nullptr; };
	cc_options o;
	if (const char *e = getenv("EBPF_CC_OFF"))
		o.off = (unsigned)strtoul(e, nullptr, 0);
	o.runmask = !set("EBPF_CC_NORUNMASK");
	o.hoist = !set("EBPF_CC_NOHOIST");
	o.short_mask = !set("EBPF_CC_NOSHORT");
	o.exit_call = set("EBPF_CC_EXITCALL");
	o.pktv = !set("EBPF_CC_NOPKTV");
	o.hash_forward = !set("EBPF_CC_NOHFWD");
	o.drop_stores = !set("EBPF_CC_KEEPSTORES");
	o.compile = !set("EBPF_JIT_NOCC");
	o.structured = !set("EBPF_JIT_NOSTRUCT");
	o.reverse_loops = !set("EBPF_JIT_NOREVLOOP");
	return o;
}

void
cc_prologue(int mode, uint16_t live, bool needs_pkt, bool structured, std::vector<uint8_t> &out)
{
	enc P{out};
	if (structured) // s7 |= 4
		P.sop2(S2_OR_B32, S_MODE, sreg(S_MODE), opnd{128 + (1u << AH_MODE_STRUCTURED)});
	if (mode == 1 && (needs_pkt || (live & (1u << 1)))) {
		// staged kernel: packet address = data + index * 64 (the kernel leaves the index in V_GIDX)
		P.vop1(V1_MOV_B32, T1, opnd{128 + 64});
		P.vop3(V3_MAD_U64_U32, V_PKT, VGPR0 + AH_V_GIDX, VGPR0 + T1, S_DATA, S_JUNK);
		P.vop1(V1_MOV_B32, V_LEN, opnd{128 + 64});
	}
	if (live & (1u << 1))
		P.vop1(V1_MOV_B64, 2, vreg(V_PKT));
	if (live & (1u << 10)) {
		P.vop2(V2_ADD_U32, 20, sreg(S_STKSTRIDE), V_STK);
		P.vop1(V1_MOV_B32, 21, sreg(S_SHARED_HI));
	}
	for (int r = 0; r < AH_NREGS; r++)
		if (r != 1 && r != 10 && (live & (1u << r)))
			P.vop1(V1_MOV_B64, 2 * r, opnd{128});
}

// VOP3 instructions this thread's compiler has emitted with two SGPR sources (a bug: see enc)
unsigned
cc_bus_violations()
{
	return g_bus_violations;
}

void
cc_compile(const dprog_host &xl, const std::vector<dp_entry> &low, const std::vector<uint32_t> &order,
	   const std::vector<char> &entry_point, int mode, bool structured, const cc_routines &rt,
	   const std::vector<dp_map> &table, const cc_options &opt, std::vector<cc_block> &out)
{
	compiler c(xl, low, order, entry_point, mode, structured, rt, table, opt, out);
	c.count_predecessors();
	c.plan_hoists();
	c.forward_pass(false);
	c.liveness();
	c.forward_pass(true);
	const bool needs_pkt = c.needs_packet_address();
	c.drop_dead_stack_stores();
	c.emit_prologue(needs_pkt);
}
