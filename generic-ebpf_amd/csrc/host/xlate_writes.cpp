// xlate_writes.cpp — stores into map values (ebpf_gpu.h "Stores into map values"): the counter
// idiom becomes DK_CNT_STORE (fuse_counters), then analyze_writes decides which maps the stores
// may reach and how each written map's writes land (dprog_host upd_maps / hupd_maps /
// atomic_maps), whether the packet may read its own stores back (the overlay), what a program
// with loops may do, and the write log's records per path.
#include "xlate.h"

namespace xlate {

// Counter updates: three consecutive entries
//   LDX{W,DW} X = [P + off] (X != P);  ADD / SUB to X of an immediate or of a register other than
//   X (64-bit; 32-bit too for W; the reference's MOV64, which adds); STX [P + off] = X, same width
// make the STX a DK_CNT_STORE.  The pattern is on executed instructions, JA aside (the graph has
// JA folded): where the ALU or the STX entry has other predecessors (standard semantics), the
// pattern's path gets copies of its own (the graph grows: ctx.changed).
int
fuse_counters(ctx &c)
{
	dprog_host &out = c.out;
	const size_t n0 = out.entries.size();
	const pred_lists preds = preds_of(out);
	for (uint32_t i = 0; i < n0; i++) {
		const dp_entry e1 = out.entries[i];
		if (!out.annot[i].reached || !(e1.kind == EBPF_OP_LDXW || e1.kind == EBPF_OP_LDXDW) ||
		    e1.dst == e1.src)
			continue;
		const uint32_t w = e1.kind == EBPF_OP_LDXDW ? 8 : 4;
		const uint32_t j = e1.next;
		if (j >= n0)
			continue;
		const dp_entry e2 = out.entries[j];
		bool ok = false;
		if (e2.dst == e1.dst && e2.aux != DP_AUX_SYNTH)
			switch (e2.kind) {
			case EBPF_OP_ADD64_IMM: case EBPF_OP_SUB64_IMM: ok = true; break;
			case EBPF_OP_ADD64_REG: case EBPF_OP_SUB64_REG: ok = e2.src != e1.dst; break;
			case EBPF_OP_MOV64_IMM: ok = !c.std_sem; break; // (standard MOV64s are rewritten)
			case EBPF_OP_MOV64_REG: ok = !c.std_sem && e2.src != e1.dst; break;
			case EBPF_OP_ADD_IMM: case EBPF_OP_SUB_IMM: ok = w == 4; break;
			case EBPF_OP_ADD_REG: case EBPF_OP_SUB_REG: ok = w == 4 && e2.src != e1.dst; break;
			default: break;
			}
		if (!ok || e2.next >= n0)
			continue;
		const uint32_t k3 = e2.next;
		const dp_entry e3 = out.entries[k3];
		if (e3.kind != (w == 8 ? EBPF_OP_STXDW : EBPF_OP_STXW) || e3.dst != e1.src ||
		    e3.src != e1.dst || e3.off != e1.off)
			continue;
		dp_entry st = e3;
		st.kind = DK_CNT_STORE;
		st.aux = (uint16_t)w;
		st.imm = 0;
		switch (e2.kind) { // an immediate addend (the ALU's): imm = what the update adds
		case EBPF_OP_ADD64_IMM: case EBPF_OP_MOV64_IMM: case EBPF_OP_ADD_IMM:
			st.imm = e2.imm;
			st.aux |= DP_AUX_IMM;
			break;
		case EBPF_OP_SUB64_IMM: case EBPF_OP_SUB_IMM:
			st.imm = 0 - e2.imm;
			st.aux |= DP_AUX_IMM;
			break;
		default:
			break;
		}
		if (preds.count(j) == 1 && preds.count(k3) == 1) {
			out.entries[k3] = st;
			continue;
		}
		// (a merge point under standard semantics: the pattern's own copies)
		dp_entry alu = e2;
		alu.next = append(out, st);
		out.entries[i].next = append(out, alu);
		c.changed = true;
	}
	return 0;
}

namespace {

// Registers an entry reads and writes, for liveness (a read over-approximated, a write only where
// certain; an entry kind not listed reads every register).
void
reg_rw(const dp_entry &e, uint16_t *rd, uint16_t *wr)
{
	const uint16_t k = e.kind, d = (uint16_t)(1u << (e.dst & 15)), s = (uint16_t)(1u << (e.src & 15));
	*rd = 0;
	*wr = 0;
	switch (k) {
	case DK_FAULT: case DK_LOOPINIT: case DK_LOOPCNT: case DK_OVLINIT:
		return;
	case EBPF_OP_EXIT:
		*rd = 1;
		return;
	case DK_CALL_LOOKUP: case DK_CALL_HDELETE: // (map, key)
		*rd = 0x6;
		*wr = 1;
		return;
	case DK_CALL_UPDATE: // (map, key, value, flags)
		*rd = 0x1e;
		*wr = 1;
		return;
	case DK_CNT_STORE: case DK_XADD:
		*rd = d | s;
		return;
	case DK_MOV64R:
		*rd = s;
		*wr = d;
		return;
	case EBPF_OP_LDDW:
		*wr = d;
		return;
	default:
		break;
	}
	if (k >= DK_NEG64 && k <= DK_MOD32Z) {
		*rd = d | s;
		*wr = d;
		return;
	}
	if (k >= 0x100) {
		*rd = 0x7ff;
		return;
	}
	switch (k & 7) {
	case EBPF_CLS_LDX: *rd = s; *wr = d; return;
	case EBPF_CLS_ST: *rd = d; return;
	case EBPF_CLS_STX: *rd = d | s; return;
	case EBPF_CLS_JMP: case DP_CLS_JMP32: *rd = d | ((k & 0x08) ? s : 0); return;
	default: *rd = d | ((k & 0x08) ? s : 0); *wr = d; return; // ALU / ALU64
	}
}

// Registers live after each entry (a backward pass to a fixed point: the graph may have loops).
std::vector<uint16_t>
live_out(const dprog_host &out)
{
	const size_t n = out.entries.size();
	std::vector<uint16_t> rd(n), wr(n), lin(n, 0), lout(n, 0);
	for (size_t i = 0; i < n; i++)
		reg_rw(out.entries[i], &rd[i], &wr[i]);
	for (bool changed = true; changed;) {
		changed = false;
		for (size_t i = n; i-- > 0;) {
			uint16_t o = 0;
			for (const edge s : succs(out, (uint32_t)i))
				o |= lin[s.to];
			const uint16_t in = rd[i] | (uint16_t)(o & ~wr[i]);
			if (o != lout[i] || in != lin[i]) {
				lout[i] = o;
				lin[i] = in;
				changed = true;
			}
		}
	}
	return lout;
}

// A reached store that may go into a map value (ST, STX, a counter update — *add — or XADD),
// and the pointer it stores through.  (The stack and the packet are never a map's values.)
bool
is_vsite(const dprog_host &out, size_t i, bool *add, av *base)
{
	const dp_entry &e = out.entries[i];
	const uint8_t cls = e.kind < 0x100 ? (e.kind & 7) : 0xff;
	*add = e.kind == DK_CNT_STORE || e.kind == DK_XADD;
	if (!out.annot[i].reached || (!*add && cls != EBPF_CLS_ST && cls != EBPF_CLS_STX))
		return false;
	*base = out.annot[i].in[e.dst];
	return base->kind != AV_STACK && base->kind != AV_CTX && base->kind != AV_CTXV;
}

bool
is_vsite(const dprog_host &out, size_t i)
{
	bool add;
	av base;
	return is_vsite(out, i, &add, &base);
}

uint32_t
store_size(const dp_entry &e)
{
	if (e.kind == DK_CNT_STORE || e.kind == DK_XADD)
		return e.aux & DP_AUX_SIZE;
	const uint32_t z = e.kind & 0x18;
	return z == 0x00 ? 4 : z == 0x08 ? 2 : z == 0x10 ? 1 : 8;
}

// Sites that log: update and delete calls, every store, and counter updates unless all the maps
// they may reach are atomic
bool
logs(const dprog_host &out, size_t i)
{
	const dp_entry &e = out.entries[i];
	if (e.kind == DK_CALL_UPDATE || e.kind == DK_CALL_HDELETE)
		return true;
	bool add;
	av b;
	if (!is_vsite(out, i, &add, &b))
		return false;
	if (!add)
		return true;
	for (size_t m : reach(out, b))
		if (!contains(out.atomic_maps, m))
			return true;
	return false;
}

// Job 1: the class of every map a store may reach.  Per map: stores, counter updates, counter
// widths, and whether every counter update is through that map's lookup result at an offset
// aligned for every key
void
class_written_maps(dprog_host &out)
{
	const size_t n = out.entries.size(), nm = out.maps.size();
	std::vector<uint32_t> nset(nm, 0), nadd(nm, 0), widths(nm, 0);
	std::vector<char> exact(nm, 1);
	out.vstore_sites = 0;
	for (size_t i = 0; i < n; i++) {
		bool add;
		av b;
		if (!is_vsite(out, i, &add, &b))
			continue;
		out.vstore_sites++;
		const dp_entry &e = out.entries[i];
		const uint32_t w = store_size(e);
		const reach maps(out, b);
		for (size_t m : maps) {
			if (!add) {
				nset[m]++;
				continue;
			}
			nadd[m]++;
			widths[m] |= w;
			const int64_t o = b.off + e.off;
			if (!maps.known || out.maps[m]->value_size % w || ((o % w) + w) % w)
				exact[m] = 0;
		}
	}
	for (size_t m = 0; m < nm; m++) {
		if (nset[m] == 0 && nadd[m] == 0)
			continue;
		if (out.maps[m]->is_hashtable()) {
			put(out.hupd_maps, m);
		} else if (nadd[m] == 0) {
			put(out.upd_maps, m); // stores (and update calls): byte winners on the device
			put(out.vstore_maps, m);
		} else if (nset[m] == 0 && !contains(out.upd_maps, m) && exact[m] &&
			   (widths[m] == 4 || widths[m] == 8)) {
			put(out.atomic_maps, m);
			out.atomic_width.push_back((uint8_t)widths[m]);
		} else {
			drop(out.upd_maps, m);
			put(out.hupd_maps, m);
		}
	}
}

// Job 2: may a load read a value the packet stored before it (the overlay)?
void
reads_own_stores(dprog_host &out)
{
	const size_t n = out.entries.size();
	// a forward pass: `stored` after an entry when any path to it passed a store into a map value
	std::vector<char> stored(n, 0), seen(n, 0);
	std::vector<uint32_t> work{out.start};
	seen[out.start] = 1;
	while (!work.empty()) {
		const uint32_t id = work.back();
		work.pop_back();
		const char after = stored[id] || is_vsite(out, id);
		for (const edge s : succs(out, id))
			if (!seen[s.to] || (after && !stored[s.to])) {
				seen[s.to] = 1;
				stored[s.to] = stored[s.to] || after;
				work.push_back(s.to);
			}
	}
	// A counter update whose register nobody reads after its STX needs no value the packet sees:
	// its addition is the same whatever was loaded, so neither it nor the idiom's LDX makes the
	// packet read its own stores back
	const std::vector<uint16_t> lout = live_out(out);
	auto cnt_dead = [&](size_t k) {
		const dp_entry &c = out.entries[k];
		return c.kind == DK_CNT_STORE && !((lout[k] >> c.src) & 1);
	};
	auto idiom_head_dead = [&](size_t i) { // LDX i -> ALU -> CNT_STORE with a dead register
		const dp_entry &e = out.entries[i];
		if (!(e.kind == EBPF_OP_LDXW || e.kind == EBPF_OP_LDXDW) || e.next >= n)
			return false;
		const uint32_t k = out.entries[e.next].next;
		if (k >= n)
			return false;
		const dp_entry &c = out.entries[k];
		return c.kind == DK_CNT_STORE && c.src == e.dst && c.dst == e.src && c.off == e.off && cnt_dead(k);
	};
	out.vstore_overlay = false;
	for (size_t i = 0; i < n && !out.vstore_overlay; i++) {
		const dp_entry &e = out.entries[i];
		if (!out.annot[i].reached || !stored[i])
			continue;
		if (e.kind == DK_CNT_STORE) {
			out.vstore_overlay = !cnt_dead(i); // (it loaded the value it adds to)
		} else if (e.kind == DK_XADD) {
			out.vstore_overlay = (e.aux & DP_AUX_FETCH) != 0; // (it returns the old value)
		} else if (e.kind < 0x100 && (e.kind & 7) == EBPF_CLS_LDX) {
			const av &b = out.annot[i].in[e.src];
			out.vstore_overlay = b.kind != AV_STACK && b.kind != AV_CTX && b.kind != AV_CTXV &&
					     !idiom_head_dead(i);
		}
	}
}

int
refuse(dprog_host &out, const char *msg)
{
	out.error = EOPNOTSUPP;
	out.error_msg = msg;
	return EOPNOTSUPP;
}

// Job 3: programs with loops, where a path has no bound on its writes.  Counter updates are
// device atomics (an array only aligned counter updates of one width change) or records of a
// hashtable's values, which count as logged writes like every other record; the logged writes
// are capped per packet (DP_WRITES_MAX, the next one faults EBPF_FAULT_WRITES), which also bounds
// the overlay (two words per store).  An array mixing counter updates with other writes is refused
int
loop_rules(dprog_host &out)
{
	const size_t n = out.entries.size();
	bool counters = false, atomic_cnt = false;
	for (size_t i = 0; i < n; i++) {
		const dp_entry &e = out.entries[i];
		if (!out.annot[i].reached || !(e.kind == DK_CNT_STORE || e.kind == DK_XADD))
			continue;
		counters = true;
		if (!out.has_loops)
			continue;
		for (size_t m : reach(out, out.annot[i].in[e.dst])) {
			const bool atomic = contains(out.atomic_maps, m);
			atomic_cnt = atomic_cnt || atomic;
			if (!atomic && !out.maps[m]->is_hashtable())
				return refuse(out, "in a program with loops, counter updates must go to a hashtable or to "
						   "an array map that only aligned counter updates of one width change (run "
						   "this one with ebpf_prog_run)");
		}
	}
	// A program with loops that reads its counter updates back (slot_reads_counters: a live
	// idiom register, XADD with BPF_FETCH) keeps the packet's view of them in the overlay, 32
	// words (DP_OVL_MAX; the store that needs one more faults EBPF_FAULT_WRITES).  A read-back
	// of another form (a later load of a counter's word) is refused when device atomics take
	// counter updates (they are not counted, so nothing else bounds the overlay); a hashtable's
	// counter records are counted, so its overlay holds at most two words per logged write
	if (out.has_loops && counters && out.reads_counters)
		out.vstore_overlay = true;
	else if (out.has_loops && atomic_cnt && out.vstore_overlay)
		return refuse(out, "in a program with loops, the packet may read back the values its counter "
				   "updates change only through the idiom's register or XADD with BPF_FETCH (run "
				   "this one with ebpf_prog_run)");
	return 0;
}

// Job 4: per path, the records the log needs and the stores the overlay holds.
int
size_log_and_overlay(dprog_host &out)
{
	const size_t n = out.entries.size();
	std::vector<uint32_t> best(n, 0), bests(n, 0);
	std::vector<uint8_t> state(n, 0);
	std::vector<uint32_t> st{out.start};
	while (!st.empty()) {
		const uint32_t id = st.back();
		if (state[id] == 0) {
			state[id] = 1;
			for (const edge s : succs(out, id))
				if (state[s.to] == 0)
					st.push_back(s.to);
			continue;
		}
		st.pop_back();
		if (state[id] == 2)
			continue;
		uint32_t m = 0, ms = 0;
		for (const edge s : succs(out, id)) {
			m = std::max(m, best[s.to]);
			ms = std::max(ms, bests[s.to]);
		}
		best[id] = m + (logs(out, id) ? 1u : 0u);
		bests[id] = ms + (is_vsite(out, id) ? 1u : 0u);
		state[id] = 2;
	}
	out.max_updates = best[out.start];
	out.ovl_entries = out.vstore_overlay ? 2 * bests[out.start] : 0;
	// A loop-free program's log and overlay are sized by its path counts: every write it reaches
	// lands, as in the reference (ebpf_interpreter.c:343-366, ebpf_map.c:101-108).  Only a loop
	// has no per-path bound; its writes are capped (DP_WRITES_MAX)
	out.write_cap = false;
	if (out.has_loops) { // (the path counts above do not bound a loop)
		bool logging = false;
		for (size_t i = 0; i < n && !logging; i++)
			logging = out.annot[i].reached && logs(out, i);
		out.write_cap = logging;
		out.max_updates = logging ? DP_WRITES_MAX : 0;
		out.ovl_entries = out.vstore_overlay ? 2 * DP_WRITES_MAX : 0;
	}
	// (a loop-free path with more than DP_OVL_MAX / 2 stores read back runs on the portable
	// interpreter with its overlay spilled to memory, 16 B an entry per lane)
	if (out.ovl_entries > DP_OVL_SPILL_MAX)
		return refuse(out, "the program stores into map values and reads them back more often on one "
				   "path than the device overlay holds (run it with ebpf_prog_run)");
	return 0;
}

} // namespace

int
analyze_writes(ctx &c)
{
	class_written_maps(c.out);
	reads_own_stores(c.out);
	if (int err = loop_rules(c.out))
		return err;
	return size_log_and_overlay(c.out);
}

} // namespace xlate
