// xlate_maps.cpp — the program's map table and its map helpers: which maps the program names
// (collect_maps), the compare chains that make a map known only at run time a translation-time
// constant (lookup_chains, update_chains), and what update / delete become once it is one
// (resolve_updates).
#include "xlate.h"

namespace xlate {

// The device map table: LDDW immediates that are live maps of the program's env, then the maps
// the program depends on.  Also the deepest stack store (max_stack).
int
collect_maps(ctx &c)
{
	dprog_host &out = c.out;
	struct ebpf_env *ee = c.ep->eo.eo_ee;
	const struct ebpf_map *unsupported = nullptr;
	auto add_map = [&](struct ebpf_map *m) {
		if (map_device_layout_of(m).bytes == 0) {
			// device batches resolve array and hashtable maps (percpu ones included); a
			// map with no device form runs on the CPU path only (ebpf_prog_run)
			unsupported = m;
			return;
		}
		if (std::find(out.maps.begin(), out.maps.end(), m) == out.maps.end())
			out.maps.push_back(m);
	};
	for (const dp_entry &e : out.entries) {
		if (e.kind == EBPF_OP_LDDW) {
			auto *cand = reinterpret_cast<struct ebpf_map *>((uintptr_t)e.imm);
			if (ee->maps.count(cand))
				add_map(cand);
		}
		const uint8_t cls = e.kind < 0x100 ? (e.kind & 7) : 0xff;
		if ((cls == EBPF_CLS_ST || cls == EBPF_CLS_STX) && e.dst == EBPF_R10 && e.off < 0 &&
		    (uint32_t)(-e.off) > out.max_stack)
			out.max_stack = (uint32_t)(-e.off);
	}
	for (uint32_t i = 0; i < c.ep->ndep_maps; i++)
		if (ee->maps.count(c.ep->dep_maps[i]))
			add_map(c.ep->dep_maps[i]);
	if (unsupported != nullptr) {
		out.error = EOPNOTSUPP;
		out.error_msg = std::string("the program uses a ") + unsupported->emt->name +
				" map with no device form (hashtable keys over 65535 bytes or a table over 64 GiB; "
				"run it with "
				"ebpf_prog_run)";
		return EOPNOTSUPP;
	}
	c.changed = true; // (the table is known: the first dataflow)
	return 0;
}

namespace {

uint32_t
compare(dprog_host &out, uint16_t kind, uint8_t reg, uint64_t imm, uint32_t taken, uint32_t next)
{
	dp_entry j = entry(kind);
	j.dst = reg;
	j.imm = imm;
	j.target = taken;
	j.next = next;
	return append(out, j);
}

// The call at entry i, its map known only at run time, becomes a ladder on r1: one 64-bit JEQ
// per map of the table (per hashtable: hash_only), taken into a copy of the call — where the
// dataflow then knows the map — and ending at `chain`.  The first compare takes the call's place.
void
ladder(dprog_host &out, size_t i, uint32_t chain, bool hash_only)
{
	const dp_entry call = out.entries[i];
	for (size_t m = out.maps.size(); m-- > 0;) {
		if (hash_only && !out.maps[m]->is_hashtable())
			continue;
		const uint32_t copy = append(out, call);
		chain = compare(out, EBPF_OP_JEQ_IMM, EBPF_R1, (uint64_t)(uintptr_t)out.maps[m], copy, chain);
	}
	out.entries[i] = out.entries[chain];
	out.entries[chain].kind = DK_FAULT; // (its copy is unreachable)
	out.entries[chain].aux = EBPF_FAULT_SLOT;
}

} // namespace

// A hashtable lookup runs a probe specialised for its map.  A lookup whose map is known only at
// run time, in a program with hashtables, becomes a compare chain on r1: one JEQ per hashtable of
// the table, ending in the generic lookup (array maps, NULL, not a map).  Its successor then has
// several predecessors: the dataflow runs again over the graph.
int
lookup_chains(ctx &c)
{
	dprog_host &out = c.out;
	if (std::none_of(out.maps.begin(), out.maps.end(), [](const struct ebpf_map *m) { return m->is_hashtable(); }))
		return 0;
	const size_t n0 = out.entries.size();
	for (size_t i = 0; i < n0; i++) {
		if (out.entries[i].kind != DK_CALL_LOOKUP || !out.annot[i].reached ||
		    out.annot[i].in[1].kind == AV_CONST)
			continue;
		ladder(out, i, append(out, out.entries[i]), true);
		c.changed = true;
	}
	return 0;
}

// Map-writing helpers whose map is known only at run time (r1 not a translation-time constant of
// the map table): a compare chain on r1 as for lookups, over every map of the table; when none
// matches, the reference's argument checks come first (ebpf_map.c:101-108: em, key or value
// NULL, or flags > EBPF_EXIST -> EINVAL; delete :130-136: em or key NULL -> EINVAL), then the
// call dereferences a pointer that is not a map of this env: EBPF_FAULT_BAD_MAP.
int
update_chains(ctx &c)
{
	dprog_host &out = c.out;
	const size_t n0 = out.entries.size();
	for (size_t i = 0; i < n0; i++) {
		if (out.entries[i].kind != DK_CALL_UPDATE || !out.annot[i].reached ||
		    map_index_of(out, out.annot[i].in[1]) >= 0) // (a map of the table: resolve_updates)
			continue;
		const bool del = out.entries[i].aux == DP_AUX_DELETE;
		dp_entry x = entry(EBPF_OP_LDDW); // r0 = EINVAL, then the call's successor
		x.imm = EINVAL;
		x.next = out.entries[i].next;
		const uint32_t einval = append(out, x);
		uint32_t chain = append(out, fault_entry(EBPF_FAULT_BAD_MAP));
		if (!del) {
			chain = compare(out, EBPF_OP_JGT_IMM, EBPF_R4, EBPF_EXIST, einval, chain);
			chain = compare(out, EBPF_OP_JEQ_IMM, EBPF_R3, 0, einval, chain);
		}
		chain = compare(out, EBPF_OP_JEQ_IMM, EBPF_R2, 0, einval, chain);
		chain = compare(out, EBPF_OP_JEQ_IMM, EBPF_R1, 0, einval, chain);
		ladder(out, i, chain, false);
		c.changed = true;
	}
	return 0;
}

// Map-writing helpers, the map now a translation-time constant of the table.  delete on an
// array map is EINVAL whatever its arguments (ebpf_map.c delete -> ebpf_map_array.c:246-250): a
// constant; on a hashtable it becomes DK_CALL_HDELETE.  update keeps its entry, aux = the map's
// table index (its routine checks the arguments at run time).
int
resolve_updates(ctx &c)
{
	dprog_host &out = c.out;
	for (size_t i = 0; i < out.entries.size(); i++) {
		dp_entry &e = out.entries[i];
		if (e.kind != DK_CALL_UPDATE || !out.annot[i].reached)
			continue;
		const int mi = map_index_of(out, out.annot[i].in[1]);
		if (mi < 0) { // (a constant that is not a map of the table)
			e.kind = DK_FAULT;
			e.aux = EBPF_FAULT_BAD_MAP;
			continue;
		}
		const bool hash = out.maps[mi]->is_hashtable();
		if (e.aux != DP_AUX_DELETE) {
			e.aux = (uint16_t)mi;
			put(hash ? out.hupd_maps : out.upd_maps, (size_t)mi);
		} else if (hash) {
			e.kind = DK_CALL_HDELETE; // (the key is logged; the routine checks it)
			e.aux = (uint16_t)mi;
			put(out.hupd_maps, (size_t)mi);
		} else {
			e.kind = EBPF_OP_LDDW;
			e.dst = 0;
			e.imm = EINVAL;
		}
	}
	return 0;
}

} // namespace xlate
