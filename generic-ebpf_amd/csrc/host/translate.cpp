// translate.cpp — reference bytecode → device program (dprog.h).
//
// The reference interpreter's next slot depends on (slot i, counter p):  "inst = inst + pc++"
// (sys/dev/ebpf/ebpf_interpreter.c:39), a taken jump adds its offset to p (:210 etc.) and LDDW
// adds one more (:341).  Starting from (0, 1) — the first fetch is slot 0 with pc already 1 —
//     plain:  (i, p) -> (i + p, p + 1)      LDDW: (i, p) -> (i + p + 1, p + 2)
//     taken:  (i, p) -> (i + p', p' + 1)    with p' = p + off  (u32 arithmetic)
// This file enumerates the reachable states and emits one dp_entry per state with explicit
// successors, so device code never does slot arithmetic.  Straight-line runs are emitted
// contiguously (fallthrough successor = index + 1) and taken sides after them.
//
// Under this rule a state (j, q) has exactly one possible predecessor slot (j - q + 1), so the
// state graph is a tree plus self-loops; a self-loop (a jump whose successor is its own state)
// is the only way the reference spins forever, and becomes an EBPF_FAULT_LOOP entry.
//
// translate_program then runs the passes of xlate.h over that graph, in order: the map table
// (xlate_maps.cpp), the pointer-provenance dataflow (xlate_dataflow.cpp, run again whenever a pass
// changed the graph), the run-time-map compare chains and update / delete resolution
// (xlate_maps.cpp), counted loops (xlate_loops.cpp), counter updates and the map-write analysis
// (xlate_writes.cpp, with the slot-graph restatement of xlate_slots.cpp), the overlay's start
// entry, and pinning the maps.  EBPF_XLATE_DUMP=file writes the result (xlate_dump.cpp).
#include "xlate.h"

#include <unordered_map>

namespace xlate {

bool
valid_op(uint8_t op)
{
	static const uint8_t ops[] = {
	    0x04, 0x0c, 0x14, 0x1c, 0x24, 0x2c, 0x34, 0x3c, 0x44, 0x4c, 0x54, 0x5c, 0x64, 0x6c,
	    0x74, 0x7c, 0x84, 0x94, 0x9c, 0xa4, 0xac, 0xb4, 0xbc, 0xc4, 0xcc, 0xd4, 0xdc, 0x07,
	    0x0f, 0x17, 0x1f, 0x27, 0x2f, 0x37, 0x3f, 0x47, 0x4f, 0x57, 0x5f, 0x67, 0x6f, 0x77,
	    0x7f, 0x87, 0x97, 0x9f, 0xa7, 0xaf, 0xb7, 0xbf, 0xc7, 0xcf, 0x61, 0x69, 0x71, 0x79,
	    0x62, 0x6a, 0x72, 0x7a, 0x63, 0x6b, 0x73, 0x7b, 0x18, 0x05, 0x15, 0x1d, 0x25, 0x2d,
	    0x35, 0x3d, 0x45, 0x4d, 0x55, 0x5d, 0x65, 0x6d, 0x75, 0x7d, 0x85, 0x95, 0xa5, 0xad,
	    0xb5, 0xbd, 0xc5, 0xcd, 0xd5, 0xdd};
	static bool tab[256];
	static bool init = [] {
		for (uint8_t o : ops)
			tab[o] = true;
		return true;
	}();
	(void)init;
	return tab[op];
}

bool
uses_dst(uint8_t op)
{
	return !(op == EBPF_OP_JA || op == EBPF_OP_CALL || op == EBPF_OP_EXIT);
}

bool
uses_src(uint8_t op)
{
	uint8_t cls = op & 7;
	if (cls == EBPF_CLS_LDX || cls == EBPF_CLS_STX)
		return true;
	if ((cls == EBPF_CLS_ALU || cls == EBPF_CLS_ALU64 || cls == EBPF_CLS_JMP) && (op & 0x08))
		return !(op == EBPF_OP_BE || op == EBPF_OP_CALL || op == EBPF_OP_EXIT);
	return false;
}

namespace {

struct Translator {
	const struct ebpf_inst *code;
	uint64_t nslots;
	const struct ebpf_config *ec;
	dprog_host &out;
	std::unordered_map<uint64_t, uint32_t> state_id;
	uint32_t fault_id[EBPF_FAULT_MAX];
	std::vector<std::pair<uint32_t, uint64_t>> pending; // (entry, state) to fill
	std::vector<std::pair<uint32_t, uint64_t>> loop_next; // (LOOPCNT entry, state it leads to)
	bool overflow = false;
	bool std_mode = false; // EBPF_SEM_STANDARD: sequential pc, the state is the slot alone

	Translator(const struct ebpf_inst *c, uint64_t n, const struct ebpf_config *e, dprog_host &o,
		   bool std_sem)
	    : code(c), nslots(n), ec(e), out(o), std_mode(std_sem)
	{
		for (auto &f : fault_id)
			f = UINT32_MAX;
	}

	static uint64_t key(uint64_t idx, uint32_t pc) { return (idx << 32) | pc; }

	uint32_t new_entry()
	{
		if (out.entries.size() >= kMaxEntries) {
			overflow = true;
			return 0;
		}
		return append(out, entry(0));
	}

	uint32_t fault(int code)
	{
		if (fault_id[code] == UINT32_MAX) {
			const uint32_t id = new_entry();
			out.entries[id].kind = DK_FAULT;
			out.entries[id].aux = (uint16_t)code;
			fault_id[code] = id;
		}
		return fault_id[code];
	}

	// A taken backward jump to slot `idx` (standard semantics): a LOOPCNT entry on the edge,
	// which counts the jump and continues at the target's entry (resolved in run()).
	uint32_t loop_edge(uint64_t idx)
	{
		// (a jump before slot 0 wraps: past the program, not a state key, and not a loop — it
		// faults when taken, so nothing is counted and has_loops stays as it is)
		if (idx >= nslots)
			return fault(EBPF_FAULT_SLOT);
		const uint32_t id = new_entry();
		out.entries[id].kind = DK_LOOPCNT;
		out.has_loops = true;
		loop_next.push_back({id, key(idx, 0)});
		return id;
	}

	// Entry for state (idx, pc), following JA chains.  New states are queued for filling.
	uint32_t get(uint64_t idx, uint32_t pc, bool *created)
	{
		*created = false;
		std::vector<uint64_t> aliases;
		uint32_t id = UINT32_MAX;
		for (uint64_t hops = 0;; hops++) {
			if (idx >= nslots) {
				id = fault(EBPF_FAULT_SLOT);
				break;
			}
			auto it = state_id.find(key(idx, pc));
			if (it != state_id.end()) {
				id = it->second;
				break;
			}
			const struct ebpf_inst &in = code[idx];
			if (std_mode && in.opcode == EBPF_OP_JA && hops <= nslots + 2) {
				aliases.push_back(key(idx, pc));
				const uint64_t nidx = idx + 1 + (uint64_t)(int64_t)in.offset;
				if (nidx == idx) {
					id = fault(EBPF_FAULT_LOOP);
					break;
				}
				if (in.offset < 0) { // a backward JA: counted
					id = loop_edge(nidx);
					break;
				}
				idx = nidx;
				continue;
			}
			if (in.opcode == EBPF_OP_JA && hops <= nslots + 2) {
				uint32_t np = pc + (uint32_t)(int32_t)in.offset;
				uint64_t nidx = idx + np;
				aliases.push_back(key(idx, pc));
				if (nidx == idx && np + 1 == pc) {
					id = fault(EBPF_FAULT_LOOP);
					break;
				}
				idx = nidx;
				pc = np + 1;
				continue;
			}
			if (in.opcode == EBPF_OP_JA) { // pathological chain
				id = fault(EBPF_FAULT_LOOP);
				break;
			}
			id = new_entry();
			state_id[key(idx, pc)] = id;
			pending.push_back({id, key(idx, pc)});
			*created = true;
			break;
		}
		for (uint64_t a : aliases)
			state_id[a] = id;
		return id;
	}

	// Standard semantics: entries for the operations whose meaning differs from the reference's
	// (returns true when `e` is complete; its successor is the next slot).
	bool std_rewrite(dp_entry &e, const struct ebpf_inst &in)
	{
		const uint8_t op = in.opcode;
		const uint64_t sx = (uint64_t)(int64_t)in.imm, zx = (uint64_t)(uint32_t)in.imm;
		switch (op) {
		case EBPF_OP_MOV64_IMM: e.kind = EBPF_OP_LDDW; e.imm = sx; return true;
		case EBPF_OP_MOV64_REG: e.kind = DK_MOV64R; return true;
		case EBPF_OP_NEG64: e.kind = DK_NEG64; return true;
		case EBPF_OP_NEG: e.kind = DK_NEG32; return true;
		case EBPF_OP_ARSH64_IMM: e.kind = DK_ARSH64I; e.imm = sx & 63; return true;
		case EBPF_OP_ARSH64_REG: e.kind = DK_ARSH64R; return true;
		case EBPF_OP_ARSH_IMM: e.kind = DK_ARSH32I; e.imm = zx & 31; return true;
		case EBPF_OP_ARSH_REG: e.kind = DK_ARSH32R; return true;
		case EBPF_OP_DIV64_REG: e.kind = DK_DIV64Z; return true;
		case EBPF_OP_MOD64_REG: e.kind = DK_MOD64Z; return true;
		case EBPF_OP_DIV_REG: e.kind = DK_DIV32Z; return true;
		case EBPF_OP_MOD_REG: e.kind = DK_MOD32Z; return true;
		case EBPF_OP_DIV64_IMM: // by a zero immediate: dst = 0
			if (sx != 0)
				return false;
			e.kind = EBPF_OP_LDDW;
			e.imm = 0;
			return true;
		case EBPF_OP_MOD64_IMM: // by a zero immediate: dst unchanged (dst += 0)
			if (sx != 0)
				return false;
			e.kind = EBPF_OP_ADD64_IMM;
			e.imm = 0;
			e.aux = DP_AUX_SYNTH; // (no counter update, fuse_counters)
			return true;
		case EBPF_OP_DIV_IMM: // 32-bit: dst = 0
			if (zx != 0)
				return false;
			e.kind = EBPF_OP_MOV_IMM;
			e.imm = 0;
			return true;
		case EBPF_OP_MOD_IMM: // 32-bit: dst = u32(dst)
			if (zx != 0)
				return false;
			e.kind = EBPF_OP_MOV_REG;
			e.src = e.dst;
			return true;
		default:
			return false;
		}
	}

	static bool valid_jmp32(uint8_t op)
	{
		switch (op & 0xf0) {
		case 0x10: case 0x20: case 0x30: case 0x40: case 0x50: case 0x60: case 0x70:
		case 0xa0: case 0xb0: case 0xc0: case 0xd0:
			return true;
		default:
			return false;
		}
	}

	// A CALL, resolved against the env's helper table at translation time: the entry's kind, or
	// the fault code
	int call_entry(dp_entry &e, int32_t imm)
	{
		const struct ebpf_helper_type *h = (imm >= 0 && imm < EBPF_TYPE_MAX) ? ec->helper_types[imm] : nullptr;
		if (h == nullptr)
			return EBPF_FAULT_HELPER;
		if (h == &eht_map_lookup_elem) {
			e.kind = DK_CALL_LOOKUP;
		} else if (h == &eht_map_update_elem || h == &eht_map_delete_elem) {
			// resolved against the map table after the dataflow pass
			e.kind = DK_CALL_UPDATE;
			e.aux = h == &eht_map_delete_elem ? DP_AUX_DELETE : 0;
		} else {
			return EBPF_FAULT_HELPER_UNSUPPORTED;
		}
		return 0;
	}

	// The taken side of the conditional jump `in` at state (idx, pc), entry id: a fault, a counted
	// back edge, or a state resolved after the straight-line runs (deferred)
	void taken_edge(uint32_t id, uint64_t idx, uint32_t pc, const struct ebpf_inst &in,
			std::vector<uint64_t> &deferred_taken, std::vector<uint32_t> &deferred_taken_entry)
	{
		const uint32_t np = pc + (uint32_t)(int32_t)in.offset;
		const uint64_t tidx = std_mode ? idx + 1 + (uint64_t)(int64_t)in.offset : idx + np;
		const uint32_t tpc = std_mode ? 0 : np + 1;
		if (tidx == idx && tpc == pc) {
			const uint32_t f = fault(EBPF_FAULT_LOOP); // (may grow entries)
			out.entries[id].target = f;
		} else if (tidx >= nslots) {
			// (before it becomes a state key: key() keeps 32 bits of the slot, and a
			// taken jump whose u32 pc wrapped lands 2^32 slots on — past the program)
			const uint32_t f = fault(EBPF_FAULT_SLOT);
			out.entries[id].target = f;
		} else if (std_mode && in.offset < 0) {
			const uint32_t c = loop_edge(tidx); // (grows entries too)
			out.entries[id].target = c;
		} else {
			deferred_taken.push_back(key(tidx, tpc));
			deferred_taken_entry.push_back(id);
		}
	}

	// Fill one entry; returns the fallthrough successor if it was newly created (so the
	// caller continues the straight-line run), else UINT32_MAX.
	void fill(uint32_t id, uint64_t idx, uint32_t pc, std::vector<uint64_t> &deferred_taken,
		  std::vector<uint32_t> &deferred_taken_entry, uint32_t *next_new)
	{
		*next_new = UINT32_MAX;
		const struct ebpf_inst &in = code[idx];
		uint8_t op = in.opcode;
		dp_entry &e = out.entries[id];
		auto make_fault = [&](int c) {
			dp_entry &x = out.entries[id];
			x.kind = DK_FAULT;
			x.aux = (uint16_t)c;
		};
		const bool jmp32 = std_mode && (op & 7) == DP_CLS_JMP32;
		// XADD (standard semantics only: the reference has no case for it, ebpf_interpreter.c:
		// 367-369): imm BPF_ADD (0) or BPF_ADD | BPF_FETCH (1)
		const bool xadd = std_mode && (op == 0xc3 || op == 0xdb);
		if (jmp32 ? !valid_jmp32(op) : !(valid_op(op) || xadd) || (xadd && in.imm != 0 && in.imm != 1)) {
			make_fault(EBPF_FAULT_BAD_OPCODE);
			return;
		}
		if (jmp32 ? (in.dst >= EBPF_REG_MAX || ((op & 0x08) && in.src >= EBPF_REG_MAX))
			  : ((uses_dst(op) && in.dst >= EBPF_REG_MAX) ||
			     (uses_src(op) && in.src >= EBPF_REG_MAX))) {
			make_fault(EBPF_FAULT_BAD_REG);
			return;
		}
		e.kind = op;
		e.dst = in.dst;
		e.src = in.src;
		e.off = in.offset;
		uint8_t cls = op & 7;
		uint64_t sx = (uint64_t)(int64_t)in.imm;
		uint64_t zx = (uint64_t)(uint32_t)in.imm;
		uint64_t next_idx = std_mode ? idx + 1 : idx + pc;
		uint32_t next_pc = std_mode ? 0 : pc + 1;
		if (std_mode && std_rewrite(e, in)) {
			bool created;
			uint32_t n = get(next_idx, next_pc, &created);
			out.entries[id].next = n;
			if (created)
				*next_new = n;
			return;
		}
		if (jmp32)
			cls = EBPF_CLS_JMP; // (a conditional jump; the entry keeps its class-6 opcode)
		switch (cls) {
		case EBPF_CLS_ALU: {
			uint8_t alu = op & 0xf0;
			if ((alu == EBPF_DIV || alu == EBPF_MOD) && !(op & 0x08) && zx == 0) {
				make_fault(EBPF_FAULT_DIV_ZERO);
				return;
			}
			e.imm = (alu == EBPF_LSH || alu == EBPF_RSH || alu == EBPF_ARSH) && !(op & 0x08)
				    ? (zx & 31)
				    : zx;
			if (op == EBPF_OP_LE || op == EBPF_OP_BE)
				e.imm = sx;
			break;
		}
		case EBPF_CLS_ALU64: {
			uint8_t alu = op & 0xf0;
			if ((alu == EBPF_DIV || alu == EBPF_MOD) && !(op & 0x08) && sx == 0) {
				make_fault(EBPF_FAULT_DIV_ZERO);
				return;
			}
			e.imm = (alu == EBPF_LSH || alu == EBPF_RSH || alu == EBPF_ARSH) && !(op & 0x08)
				    ? (sx & 63)
				    : sx;
			break;
		}
		case EBPF_CLS_LD: // LDDW (the only LD-class opcode dispatched)
			if (idx + 1 >= nslots) {
				make_fault(EBPF_FAULT_SLOT);
				return;
			}
			e.imm = zx | ((uint64_t)(uint32_t)code[idx + 1].imm << 32);
			next_idx = std_mode ? idx + 2 : idx + pc + 1;
			next_pc = std_mode ? 0 : pc + 2;
			break;
		case EBPF_CLS_ST:
			e.imm = sx;
			if (in.dst != EBPF_R10)
				out.writes_memory = true;
			break;
		case EBPF_CLS_STX:
			if (in.dst != EBPF_R10)
				out.writes_memory = true;
			if (xadd) {
				e.kind = DK_XADD;
				e.aux = (uint16_t)((op == 0xdb ? 8 : 4) | (in.imm == 1 ? DP_AUX_FETCH : 0));
				out.writes_memory = true;
			}
			break;
		case EBPF_CLS_LDX:
			break;
		case EBPF_CLS_JMP:
			if (op == EBPF_OP_EXIT)
				return;
			if (op == EBPF_OP_CALL) {
				if (const int f = call_entry(e, in.imm)) {
					make_fault(f);
					return;
				}
				break;
			}
			e.imm = jmp32 ? zx : sx;
			taken_edge(id, idx, pc, in, deferred_taken, deferred_taken_entry); // (no `e` after this)
			break;
		default:
			make_fault(EBPF_FAULT_BAD_OPCODE);
			return;
		}
		bool created;
		uint32_t n = get(next_idx, next_pc, &created);
		out.entries[id].next = n;
		if (created)
			*next_new = n;
	}

	int run()
	{
		bool created;
		out.start = get(0, 1, &created);
		std::vector<uint64_t> dt;
		std::vector<uint32_t> dte;
		size_t pi = 0, di = 0, li = 0;
		while (!overflow) {
			// pending entries are processed in creation order; a straight run is filled
			// eagerly so fallthrough successors get consecutive indices.
			if (pi < pending.size()) {
				uint32_t id = pending[pi].first;
				uint64_t k = pending[pi].second;
				pi++;
				uint32_t nn;
				fill(id, k >> 32, (uint32_t)k, dt, dte, &nn);
				continue;
			}
			if (li < loop_next.size()) {
				const uint32_t from = loop_next[li].first;
				const uint64_t k = loop_next[li].second;
				li++;
				out.entries[from].next = get(k >> 32, (uint32_t)k, &created);
				continue;
			}
			if (di >= dt.size())
				break;
			uint64_t k = dt[di];
			uint32_t from = dte[di];
			di++;
			out.entries[from].target = get(k >> 32, (uint32_t)k, &created);
		}
		// A conditional jump of offset 0 goes to the same state taken or not (reference: pc += 0
		// leaves the next state (idx + pc, pc + 1) unchanged, ebpf_interpreter.c:209-211;
		// standard: pc + 1 + 0).  Its compare has no effect, so it becomes ADD64 dst, 0: the
		// state graph keeps one edge per entry (the device's structured control flow and every
		// pass that walks the tree rely on that; fuzz_gpu.py --standard found it).
		for (dp_entry &x : out.entries) {
			// (no JA or CALL is an entry: JAs are folded, calls have kinds of their own)
			if (is_cond(x) && x.target == x.next) {
				x.kind = EBPF_OP_ADD64_IMM;
				x.imm = 0;
				x.src = 0;
				x.off = 0;
				x.aux = DP_AUX_SYNTH; // (no counter update, fuse_counters)
			}
		}
		if (!overflow && out.has_loops) { // every lane's loop count starts at 0
			const uint32_t init = new_entry();
			out.entries[init].kind = DK_LOOPINIT;
			out.entries[init].next = out.start;
			out.start = init;
		}
		if (overflow) {
			out.error = E2BIG;
			out.error_msg = "program state graph exceeds the device translation limit";
			return E2BIG;
		}
		return 0;
	}
};

} // namespace

int
enumerate_states(ctx &c)
{
	Translator t(c.code, c.nslots, c.ep->eo.eo_ee->ec, c.out, c.std_sem);
	return t.run();
}

// A program that reads its own stores into map values, or whose writes are capped, starts at an
// OVLINIT entry: every lane's overlay and write count start at 0
int
overlay_init(ctx &c)
{
	if (!c.out.vstore_overlay && !c.out.write_cap)
		return 0;
	dp_entry x = entry(DK_OVLINIT);
	x.next = c.out.start;
	c.out.start = append(c.out, x);
	c.changed = true;
	return 0;
}

// The program now pins its maps (released in prog_dtor): a device mirror must not outlive its
// map while a later batch may still read it.
int
pin_maps(ctx &c)
{
	for (struct ebpf_map *m : c.out.maps)
		m->eo.eo_ref.fetch_add(1);
	return 0;
}

} // namespace xlate

bool
prog_writes_maps(const dprog_host &xl)
{
	return xl.max_updates != 0 || !xl.atomic_maps.empty();
}

int
translate_program(struct ebpf_prog *ep, dprog_host &out)
{
	using namespace xlate;
	// (grows: the pass appends entries, and the graph may then exceed the translation limit)
	static const struct {
		int (*run)(ctx &);
		bool grows;
	} passes[] = {{enumerate_states, false}, {collect_maps, false},  {lookup_chains, true},
		      {update_chains, true},     {resolve_updates, false}, {elide_loop_count, false},
		      {fuse_counters, true},     {reads_counters, false}, {analyze_writes, false},
		      {overlay_init, false},     {pin_maps, false}};
	ctx c{ep, ep->prog, ep->prog_len / sizeof(struct ebpf_inst), ep->semantics.load() == EBPF_SEM_STANDARD,
	      out};
	// (the env's maps stay as they are from the table's collection to its pinning)
	std::lock_guard<std::mutex> g(ep->eo.eo_ee->lock);
	int err = 0;
	for (const auto &p : passes) {
		c.changed = false;
		err = p.run(c);
		if (err == 0 && p.grows && out.entries.size() >= kMaxEntries) {
			out.error_msg = "program state graph exceeds the device translation limit";
			err = out.error = E2BIG;
		}
		if (err != 0)
			break;
		if (c.changed) // (the graph changed: its annotations again)
			dataflow(out);
	}
	if (err != 0)
		out.maps.clear(); // (not pinned: nothing to release)
	xlate_dump(out, err);
	return err;
}
