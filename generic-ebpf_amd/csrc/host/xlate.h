// xlate.h — the translator's own vocabulary (translate.cpp, xlate_*.cpp; nothing else includes it):
// the entry graph's successors and predecessors, entry construction, the map table's indices,
// and the passes translate_program runs in order.
#pragma once
#include "internal.h"

#include <algorithm>

namespace xlate {

constexpr uint32_t kMaxEntries = 1u << 20;

// ---- entries
// A zeroed entry of a kind; append() returns the new entry's index.
inline dp_entry
entry(uint16_t kind)
{
	dp_entry e;
	memset(&e, 0, sizeof(e));
	e.kind = kind;
	return e;
}

inline dp_entry
fault_entry(int code)
{
	dp_entry e = entry(DK_FAULT);
	e.aux = (uint16_t)code;
	return e;
}

inline uint32_t
append(dprog_host &out, const dp_entry &e)
{
	out.entries.push_back(e);
	return (uint32_t)(out.entries.size() - 1);
}

// ---- the graph
// A conditional jump (class JMP or JMP32, the opcode kept): the one kind with two successors.
inline bool
is_cond(const dp_entry &e)
{
	const uint8_t cls = e.kind & 7;
	return e.kind < 0x100 && (cls == EBPF_CLS_JMP || cls == DP_CLS_JMP32) && e.kind != EBPF_OP_EXIT;
}

// Successor k of an entry (0: next, 1: a conditional jump's target; UINT32_MAX: none).
inline uint32_t
succ_of(const dprog_host &out, uint32_t id, int k)
{
	const dp_entry &e = out.entries[id];
	if (e.kind == DK_FAULT || e.kind == EBPF_OP_EXIT)
		return UINT32_MAX;
	if (k == 0)
		return e.next;
	return is_cond(e) ? e.target : UINT32_MAX;
}

// for (const edge s : succs(out, id)): the entry's successors inside the graph, next first.
struct edge {
	uint32_t to;
	bool taken;
};
struct edge_list {
	edge e[2];
	int n = 0;
	const edge *begin() const { return e; }
	const edge *end() const { return e + n; }
};
inline edge_list
succs(const dprog_host &out, uint32_t id)
{
	edge_list l;
	for (int k = 0; k < 2; k++) {
		const uint32_t s = succ_of(out, id, k);
		if (s < out.entries.size())
			l.e[l.n++] = {s, k == 1};
	}
	return l;
}

// Predecessors over the edges that leave reached entries: for (uint32_t p : preds.of(id)).
struct pred_lists {
	std::vector<uint32_t> first, list; // of(id) = list[first[id] .. first[id + 1])
	struct range {
		const uint32_t *b, *e;
		const uint32_t *begin() const { return b; }
		const uint32_t *end() const { return e; }
	};
	range of(uint32_t id) const { return {list.data() + first[id], list.data() + first[id + 1]}; }
	uint32_t count(uint32_t id) const { return first[id + 1] - first[id]; }
};
pred_lists preds_of(const dprog_host &out);

// ---- the map table
// Table index of the map a constant handle names, or -1.
inline int
map_index_of(const dprog_host &out, const av &a)
{
	if (a.kind == AV_CONST)
		for (size_t m = 0; m < out.maps.size(); m++)
			if ((uint64_t)a.off == (uint64_t)(uintptr_t)out.maps[m])
				return (int)m;
	return -1;
}

// for (size_t m : reach(out, base)): the table maps a store through `base` may reach — the map
// of a lookup result (known), else every map.
struct reach {
	size_t lo, hi;
	bool known;
	reach(const dprog_host &out, const av &b)
	    : lo(0), hi(out.maps.size()),
	      known((b.kind == AV_MAPVAL || b.kind == AV_MAPVAL_NULL) && b.map >= 0 &&
		    (size_t)b.map < out.maps.size())
	{
		if (known) {
			lo = (size_t)b.map;
			hi = lo + 1;
		}
	}
	struct it {
		size_t m;
		size_t operator*() const { return m; }
		void operator++() { m++; }
		bool operator!=(const it &o) const { return m != o.m; }
	};
	it begin() const { return {lo}; }
	it end() const { return {hi}; }
};

// The map-index lists of dprog_host (upd_maps, hupd_maps, ...): sets in insertion order.
inline bool
contains(const std::vector<uint16_t> &v, size_t m)
{
	return std::find(v.begin(), v.end(), (uint16_t)m) != v.end();
}

inline void
put(std::vector<uint16_t> &v, size_t m)
{
	if (!contains(v, m))
		v.push_back((uint16_t)m);
}

inline void
drop(std::vector<uint16_t> &v, size_t m)
{
	v.erase(std::remove(v.begin(), v.end(), (uint16_t)m), v.end());
}

// ---- the passes, in translate_program's order.  Each returns 0 or an errno (out.error and
// out.error_msg set); those that may change the graph say so in ctx.changed, and the driver runs
// the dataflow again.
struct ctx {
	struct ebpf_prog *ep;
	const struct ebpf_inst *code;
	uint64_t nslots;
	bool std_sem;
	dprog_host &out;
	bool changed = false;
};
int enumerate_states(ctx &c);  // translate.cpp
int collect_maps(ctx &c);      // xlate_maps.cpp (the caller holds the env's lock)
int lookup_chains(ctx &c);
int update_chains(ctx &c);
int resolve_updates(ctx &c);
int elide_loop_count(ctx &c);  // xlate_loops.cpp
int fuse_counters(ctx &c);     // xlate_writes.cpp
int reads_counters(ctx &c);    // xlate_slots.cpp
int analyze_writes(ctx &c);    // xlate_writes.cpp
int overlay_init(ctx &c);      // translate.cpp
int pin_maps(ctx &c);

void dataflow(dprog_host &out); // xlate_dataflow.cpp

// translate.cpp's checks of one slot, shared with the slot-graph restatement
bool valid_op(uint8_t op);
bool uses_dst(uint8_t op);
bool uses_src(uint8_t op);

} // namespace xlate

// xlate_dump.cpp: EBPF_XLATE_DUMP
void xlate_dump(const dprog_host &out, int err);
