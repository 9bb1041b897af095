// xlate_loops.cpp — counted loops whose budget cannot run out (standard semantics).  A program
// with one loop — one LOOPCNT entry L, reached from one conditional C on a counter X:
//   JNE X, 0 taken into L (the back edge), or JEQ X, 0 whose fall-through is L (exit test, JA back)
// — where every path from the loop head H = L.next to C decrements X by one exactly once
// (SUB64 X, 1 / ADD64 X, -1), nothing else on those paths writes X or calls a helper, and X
// enters the loop in [1, K]: the loop takes at most K - 1 backward jumps, so with K - 1 <=
// DP_LOOP_BUDGET no lane can reach EBPF_FAULT_LOOP and the count is dropped (C jumps to H
// directly; the oracle counts on and never faults either).  X's entry range comes from an
// interval pass over the loop-free graph (the back edge removed): constants, loads (0 ..
// 2^(8 size) - 1), AND / RSH / MOD / ADD / SUB with immediates, 64-bit compares with immediates
// on their edges.
#include "xlate.h"

#include <array>

namespace xlate {
namespace {

struct loop_shape {
	uint32_t L, H, C;
	uint8_t X;
	bool jne_form; // else the JEQ form
};

// The one reached LOOPCNT entry, its one predecessor and the counter that one tests.
bool
find_loop(const dprog_host &out, const pred_lists &preds, loop_shape &lp)
{
	const size_t n = out.entries.size();
	lp.L = UINT32_MAX;
	for (uint32_t i = 0; i < n; i++)
		if (out.entries[i].kind == DK_LOOPCNT && out.annot[i].reached) {
			if (lp.L != UINT32_MAX)
				return false; // (several loops: their counts add up)
			lp.L = i;
		}
	if (lp.L == UINT32_MAX)
		return false;
	lp.H = out.entries[lp.L].next;
	if (lp.H >= n || out.entries[lp.H].kind == DK_FAULT || preds.count(lp.L) == 0)
		return false;
	lp.C = *preds.of(lp.L).begin();
	for (uint32_t p : preds.of(lp.L))
		if (p != lp.C)
			return false;
	const dp_entry &c = out.entries[lp.C];
	lp.jne_form = c.kind == EBPF_OP_JNE_IMM && c.target == lp.L && c.next != lp.L;
	const bool jeq_form = c.kind == EBPF_OP_JEQ_IMM && c.next == lp.L && c.target != lp.L;
	if (!(lp.jne_form || jeq_form) || c.imm != 0 || c.dst >= EBPF_REG_MAX)
		return false;
	lp.X = c.dst;
	return true;
}

// The loop body: entries on a path H ->* C (not through L); empty when H does not reach C.
std::vector<char>
loop_body(const dprog_host &out, const pred_lists &preds, const loop_shape &lp)
{
	const size_t n = out.entries.size();
	std::vector<char> fwd(n, 0), bwd(n, 0);
	std::vector<uint32_t> st{lp.H};
	fwd[lp.H] = 1;
	while (!st.empty()) {
		const uint32_t i = st.back();
		st.pop_back();
		for (const edge s : succs(out, i))
			if (s.to != lp.L && !fwd[s.to]) {
				fwd[s.to] = 1;
				st.push_back(s.to);
			}
	}
	if (!fwd[lp.C])
		return {};
	st.push_back(lp.C);
	bwd[lp.C] = 1;
	while (!st.empty()) {
		const uint32_t i = st.back();
		st.pop_back();
		if (i == lp.H)
			continue;
		for (uint32_t p : preds.of(i))
			if (fwd[p] && !bwd[p] && p != lp.L) {
				bwd[p] = 1;
				st.push_back(p);
			}
	}
	return bwd;
}

// (writes dst: ALU, ALU64, LDX, LDDW and the standard-semantics ALU kinds)
bool
writes_reg(const dp_entry &e, uint8_t r)
{
	if (e.kind >= DK_MOV64R && e.kind <= DK_MOD32Z)
		return e.dst == r;
	if (e.kind >= 0x100)
		return true; // (calls, stores into maps, loop entries: not in a counted body)
	const uint8_t cls = e.kind & 7;
	return (cls == EBPF_CLS_ALU || cls == EBPF_CLS_ALU64 || cls == EBPF_CLS_LDX || cls == EBPF_CLS_LD) &&
	       e.dst == r;
}

// Decrements of X along the body's paths: every path H ->* C exactly one, and nothing else on
// them writes X or calls a helper.
bool
one_decrement_per_path(const dprog_host &out, const loop_shape &lp, const std::vector<char> &body)
{
	const size_t n = out.entries.size();
	const uint32_t H = lp.H;
	auto inside = [&](uint32_t s) { return body[s] && s != H; }; // (an edge of the body's DAG)
	auto is_dec = [&](const dp_entry &e) {
		return e.dst == lp.X && ((e.kind == EBPF_OP_SUB64_IMM && e.imm == 1) ||
					 (e.kind == EBPF_OP_ADD64_IMM && e.imm == ~0ull && e.aux != DP_AUX_SYNTH));
	};
	std::vector<uint32_t> order; // topological over the body (a DAG: L is its only back edge)
	std::vector<uint32_t> indeg(n, 0);
	size_t nbody = 0;
	for (uint32_t i = 0; i < n; i++) {
		if (!body[i])
			continue;
		nbody++;
		for (const edge s : succs(out, i))
			if (inside(s.to))
				indeg[s.to]++;
	}
	std::vector<uint32_t> q{H};
	while (!q.empty()) {
		const uint32_t i = q.back();
		q.pop_back();
		order.push_back(i);
		for (const edge s : succs(out, i))
			if (inside(s.to) && --indeg[s.to] == 0)
				q.push_back(s.to);
	}
	if (order.size() != nbody)
		return false;
	std::vector<int> ndec(n, -1); // -1 unknown, 0 or 1, 2 = inconsistent
	ndec[H] = 0;
	for (uint32_t i : order) {
		const dp_entry &e = out.entries[i];
		int d = ndec[i];
		if (d < 0 || d > 1)
			return false;
		if (i != lp.C) {
			if (is_dec(e))
				d++;
			else if (writes_reg(e, lp.X) || e.kind == DK_XADD)
				return false;
			if (e.kind == DK_CALL_LOOKUP || e.kind == DK_CALL_UPDATE || e.kind == DK_CALL_HDELETE)
				return false;
		}
		for (const edge s : succs(out, i)) {
			if (!inside(s.to))
				continue;
			if (ndec[s.to] < 0)
				ndec[s.to] = d;
			else if (ndec[s.to] != d)
				return false;
		}
	}
	return ndec[lp.C] == 1;
}

struct iv {
	uint64_t lo = 0, hi = ~0ull;
};
typedef std::array<iv, EBPF_REG_MAX> iv_regs;

// One entry's effect on the register ranges: r after it on the fall-through edge, t on the taken
// edge of a conditional jump (64-bit compares with an immediate refine both).
void
iv_transfer(const dp_entry &e, iv_regs &r, iv_regs &t)
{
	const uint8_t d = e.dst < EBPF_REG_MAX ? e.dst : 0;
	const uint64_t K = e.imm;
	const uint8_t cls = e.kind < 0x100 ? (e.kind & 7) : 0xff;
	const iv full;
	auto set = [&](uint64_t lo, uint64_t hi) {
		r[d].lo = lo;
		r[d].hi = hi;
	};
	switch (e.kind) {
	case EBPF_OP_LDDW: set(K, K); break;
	case EBPF_OP_MOV_IMM: set((uint32_t)K, (uint32_t)K); break;
	case DK_MOV64R: r[d] = r[e.src]; break;
	case EBPF_OP_LDXB: set(0, 0xff); break;
	case EBPF_OP_LDXH: set(0, 0xffff); break;
	case EBPF_OP_LDXW: set(0, 0xffffffffull); break;
	case EBPF_OP_AND64_IMM: set(0, std::min(r[d].hi, K)); break;
	case EBPF_OP_AND_IMM: set(0, std::min<uint64_t>(r[d].hi, K & 0xffffffffull)); break;
	case EBPF_OP_RSH64_IMM: set(r[d].lo >> (K & 63), r[d].hi >> (K & 63)); break;
	case EBPF_OP_MOD64_IMM: set(0, K - 1); break; // (K != 0: MOD by 0 was rewritten)
	case EBPF_OP_ADD64_IMM:
		if ((int64_t)K >= 0 && r[d].hi <= ~0ull - K)
			set(r[d].lo + K, r[d].hi + K);
		else if ((int64_t)K < 0 && r[d].lo >= 0 - K)
			set(r[d].lo + K, r[d].hi + K);
		else
			r[d] = full;
		break;
	case EBPF_OP_SUB64_IMM:
		if ((int64_t)K >= 0 && r[d].lo >= K)
			set(r[d].lo - K, r[d].hi - K);
		else
			r[d] = full;
		break;
	default:
		if (e.kind >= DK_MOV64R && e.kind <= DK_MOD32Z)
			r[d] = full;
		else if (e.kind >= 0x100 && e.kind != DK_LOOPINIT && e.kind != DK_OVLINIT && e.kind != DK_LOOPCNT)
			for (auto &x : r)
				x = full; // (calls, XADD fetch, ...: nothing known after)
		else if (e.kind < 0x100 && writes_reg(e, d))
			r[d] = (cls == EBPF_CLS_ALU) ? iv{0, 0xffffffffull} : full;
		break;
	}
	t = r;
	if (cls == EBPF_CLS_JMP && !(e.kind & 0x08)) {
		iv &a = r[d], &b = t[d];
		switch (e.kind) {
		case EBPF_OP_JEQ_IMM: b.lo = std::max(b.lo, K); b.hi = std::min(b.hi, K); break;
		case EBPF_OP_JGT_IMM: b.lo = std::max(b.lo, K + 1); a.hi = std::min(a.hi, K); break;
		case EBPF_OP_JGE_IMM: b.lo = std::max(b.lo, K); if (K) a.hi = std::min(a.hi, K - 1); break;
		case EBPF_OP_JLT_IMM: if (K) b.hi = std::min(b.hi, K - 1); a.lo = std::max(a.lo, K); break;
		case EBPF_OP_JLE_IMM: b.hi = std::min(b.hi, K); a.lo = std::max(a.lo, K + 1); break;
		default: break;
		}
		if (e.kind == EBPF_OP_JGT_IMM && K == ~0ull)
			b = iv{1, 0}; // (never taken)
	}
}

// X's range on the way into the loop: intervals over the graph without the back edge.
bool
counter_range_at_head(const dprog_host &out, const loop_shape &lp, iv &x)
{
	const size_t n = out.entries.size();
	std::vector<iv_regs> in(n);
	std::vector<char> have(n, 0);
	std::vector<uint32_t> indeg(n, 0);
	for (uint32_t i = 0; i < n; i++)
		if (out.annot[i].reached && i != lp.L)
			for (const edge s : succs(out, i))
				indeg[s.to]++;
	for (auto &r : in[out.start]) {
		r.lo = 0;
		r.hi = 0; // (the device zeroes r0, r2..r9, as the dataflow assumes)
	}
	in[out.start][1] = iv();
	in[out.start][10] = iv();
	have[out.start] = 1;
	std::vector<uint32_t> q{out.start};
	while (!q.empty()) {
		const uint32_t i = q.back();
		q.pop_back();
		if (i == lp.L)
			continue; // (the back edge)
		iv_regs r = in[i], t;
		iv_transfer(out.entries[i], r, t);
		for (const edge s : succs(out, i)) {
			const iv_regs &from = s.taken ? t : r;
			if (!have[s.to]) {
				in[s.to] = from;
				have[s.to] = 1;
			} else {
				for (int k = 0; k < EBPF_REG_MAX; k++) {
					in[s.to][k].lo = std::min(in[s.to][k].lo, from[k].lo);
					in[s.to][k].hi = std::max(in[s.to][k].hi, from[k].hi);
				}
			}
			if (--indeg[s.to] == 0)
				q.push_back(s.to);
		}
	}
	// H's range joined the entry edges only (the back edge was skipped); every predecessor
	// outside the loop must have been processed (indeg 0), else the graph has another cycle
	if (!have[lp.H] || indeg[lp.H] != 0)
		return false;
	x = in[lp.H][lp.X];
	return true;
}

} // namespace

// a counted loop that cannot reach the budget needs no count (EBPF_XLATE_KEEP_LOOPCNT keeps it)
int
elide_loop_count(ctx &c)
{
	dprog_host &out = c.out;
	if (!out.has_loops || getenv("EBPF_XLATE_KEEP_LOOPCNT") != nullptr)
		return 0;
	const pred_lists preds = preds_of(out);
	loop_shape lp;
	iv x;
	if (!find_loop(out, preds, lp))
		return 0;
	const std::vector<char> body = loop_body(out, preds, lp);
	if (body.empty() || !one_decrement_per_path(out, lp, body) || !counter_range_at_head(out, lp, x) ||
	    x.lo < 1 || x.hi - 1 > DP_LOOP_BUDGET)
		return 0;
	dp_entry &cm = out.entries[lp.C];
	if (lp.jne_form)
		cm.target = lp.H;
	else
		cm.next = lp.H;
	c.changed = true;
	return 0;
}

} // namespace xlate
