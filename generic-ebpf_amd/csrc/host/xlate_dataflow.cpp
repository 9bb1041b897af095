// xlate_dataflow.cpp — pointer provenance over the entry graph (internal.h av): the abstract
// values' algebra, one entry's transfer function, and the fixed point that fills dp_annot.
#include "xlate.h"

namespace xlate {
namespace {

av
mk(uint8_t kind, int64_t off = 0, int16_t map = -1)
{
	av a;
	a.kind = kind;
	a.off = off;
	a.map = map;
	return a;
}

bool
is_ptr(const av &a)
{
	return a.kind == AV_CTX || a.kind == AV_STACK || a.kind == AV_MAPVAL;
}

// a number (a constant or an AV_SCALAR): nothing in it came from a pointer
bool
is_num(const av &a)
{
	return a.kind == AV_CONST || a.kind == AV_SCALAR;
}

// dst + src for ADD64 / MOV64 (which adds, ebpf_interpreter.c:197-202)
av
add_av(const av &d, const av &s)
{
	if (d.kind == AV_CONST && s.kind == AV_CONST)
		return mk(AV_CONST, (int64_t)((uint64_t)d.off + (uint64_t)s.off));
	if (is_ptr(d) && s.kind == AV_CONST)
		return mk(d.kind, (int64_t)((uint64_t)d.off + (uint64_t)s.off), d.map);
	if (d.kind == AV_CONST && is_ptr(s))
		return mk(s.kind, (int64_t)((uint64_t)s.off + (uint64_t)d.off), s.map);
	// a packet pointer moved by a number no pointer went into (a TLV walk's length field) is
	// still a packet pointer; numbers combine into numbers
	const bool pd = d.kind == AV_CTX || d.kind == AV_CTXV, ps = s.kind == AV_CTX || s.kind == AV_CTXV;
	if ((pd && is_num(s)) || (is_num(d) && ps))
		return mk(AV_CTXV);
	if (is_num(d) && is_num(s))
		return mk(AV_SCALAR);
	return av();
}

// Two paths meet: the same value, two packet pointers (one with an unknown offset), two numbers,
// else unknown
av
meet_av(const av &a, const av &b)
{
	if (a == b)
		return a;
	const bool pa = a.kind == AV_CTX || a.kind == AV_CTXV, pb = b.kind == AV_CTX || b.kind == AV_CTXV;
	if (pa && pb)
		return mk(AV_CTXV);
	return is_num(a) && is_num(b) ? mk(AV_SCALAR) : av();
}

void
transfer(const dp_entry &e, const dprog_host &out, av r[EBPF_REG_MAX])
{
	const uint16_t k = e.kind;
	if (k == DK_FAULT || k == EBPF_OP_EXIT)
		return;
	if (k == DK_MOV64R) {
		r[e.dst] = r[e.src];
		return;
	}
	if (k >= DK_NEG64 && k <= DK_MOD32Z) { // (numbers stay numbers)
		const bool reads_src = k == DK_ARSH64R || k == DK_ARSH32R || k >= DK_DIV64Z;
		const bool num = is_num(r[e.dst]) && (!reads_src || is_num(r[e.src]));
		r[e.dst] = num ? mk(AV_SCALAR) : av();
		return;
	}
	if (k == DK_CALL_LOOKUP) {
		const int m = map_index_of(out, r[1]);
		r[0] = m >= 0 ? mk(AV_MAPVAL_NULL, 0, (int16_t)m) : av();
		// (r1..r5 keep their values: a plain C call in the reference)
		return;
	}
	if (k == DK_CALL_UPDATE || k == DK_CALL_HDELETE) { // (update or delete): an errno
		r[0] = av();
		return;
	}
	if (k == DK_LOOPINIT || k == DK_LOOPCNT || k == DK_OVLINIT || k == DK_CNT_STORE)
		return;
	if (k == DK_XADD) {
		if (e.aux & DP_AUX_FETCH) // src = the old value
			r[e.src] = av();
		return;
	}
	const uint8_t cls = k & 7;
	if (is_cond(e) || cls == EBPF_CLS_ST || cls == EBPF_CLS_STX)
		return;
	if (cls == EBPF_CLS_LDX) { // packet bytes are numbers; the stack and map values may hold pointers
		const uint8_t b = r[e.src].kind;
		r[e.dst] = (b == AV_CTX || b == AV_CTXV) ? mk(AV_SCALAR) : av();
		return;
	}
	if (k == EBPF_OP_LDDW) {
		r[e.dst] = mk(AV_CONST, (int64_t)e.imm);
		return;
	}
	const av s = (k & 0x08) ? r[e.src] : mk(AV_CONST, (int64_t)e.imm);
	av &d = r[e.dst];
	switch (k) {
	case EBPF_OP_ADD64_IMM: case EBPF_OP_ADD64_REG:
	case EBPF_OP_MOV64_IMM: case EBPF_OP_MOV64_REG:
		d = add_av(d, s);
		break;
	case EBPF_OP_SUB64_IMM: case EBPF_OP_SUB64_REG: case EBPF_OP_NEG64:
		if (s.kind == AV_CONST) {
			av neg = mk(AV_CONST, (int64_t)(0 - (uint64_t)s.off));
			d = add_av(d, neg);
		} else if (s.kind == AV_SCALAR && (d.kind == AV_CTX || d.kind == AV_CTXV || is_num(d))) {
			d = add_av(d, s); // (the sign does not matter to the kind)
		} else {
			d = av();
		}
		break;
	case EBPF_OP_MOV_IMM:
		d = mk(AV_CONST, (int64_t)(uint32_t)e.imm);
		break;
	case EBPF_OP_MOV_REG:
		d = s.kind == AV_CONST ? mk(AV_CONST, (int64_t)(uint32_t)s.off) : is_num(s) ? mk(AV_SCALAR) : av();
		break;
	case EBPF_OP_NEG:
		d = mk(AV_CONST, (int64_t)(uint32_t)(0u - (uint32_t)e.imm));
		break;
	default: // other ALU: numbers in, a number out
		d = is_num(d) && ((k & 0x08) == 0 || is_num(s)) ? mk(AV_SCALAR) : av();
		break;
	}
}

} // namespace

void
dataflow(dprog_host &out)
{
	const size_t n = out.entries.size();
	out.annot.assign(n, dp_annot());
	dp_annot init;
	for (auto &x : init.in)
		x = mk(AV_CONST, 0); // the device zeroes r0, r2..r9 (the reference leaves them undefined)
	init.in[1] = mk(AV_CTX, 0);
	init.in[10] = mk(AV_STACK, 0);
	init.reached = true;
	out.annot[out.start] = init;
	std::vector<uint32_t> work{out.start};
	std::vector<char> queued(n, 0);
	queued[out.start] = 1;
	while (!work.empty()) {
		uint32_t id = work.back();
		work.pop_back();
		queued[id] = 0;
		const dp_entry &e = out.entries[id];
		if (e.kind == DK_FAULT || e.kind == EBPF_OP_EXIT)
			continue;
		av r[EBPF_REG_MAX];
		for (int i = 0; i < EBPF_REG_MAX; i++)
			r[i] = out.annot[id].in[i];
		transfer(e, out, r);
		// the taken edge of "JEQ dst, imm" knows dst == imm (the 64-bit compare)
		av rt[EBPF_REG_MAX];
		for (int i = 0; i < EBPF_REG_MAX; i++)
			rt[i] = r[i];
		if (e.kind == EBPF_OP_JEQ_IMM && e.dst < EBPF_REG_MAX)
			rt[e.dst] = mk(AV_CONST, (int64_t)e.imm);
		// a NULL test of a lookup result: past it (JEQ 0 not taken, JNE 0 taken) it is non-NULL
		if ((e.kind == EBPF_OP_JEQ_IMM || e.kind == EBPF_OP_JNE_IMM) && e.imm == 0 &&
		    e.dst < EBPF_REG_MAX && r[e.dst].kind == AV_MAPVAL_NULL) {
			av nn = r[e.dst];
			nn.kind = AV_MAPVAL;
			if (e.kind == EBPF_OP_JEQ_IMM)
				r[e.dst] = nn; // (r feeds the fall-through edge below)
			else
				rt[e.dst] = nn;
		}
		for (const edge s : succs(out, id)) {
			const uint32_t sx = s.to;
			const av *re = s.taken ? rt : r;
			dp_annot &a = out.annot[sx];
			bool changed = false;
			if (!a.reached) {
				for (int i = 0; i < EBPF_REG_MAX; i++)
					a.in[i] = re[i];
				a.reached = true;
				changed = true;
			} else {
				for (int i = 0; i < EBPF_REG_MAX; i++) {
					const av m = meet_av(a.in[i], re[i]);
					if (m != a.in[i]) {
						a.in[i] = m;
						changed = true;
					}
				}
			}
			if (changed && !queued[sx]) {
				queued[sx] = 1;
				work.push_back(sx);
			}
		}
	}
}

pred_lists
preds_of(const dprog_host &out)
{
	const size_t n = out.entries.size();
	pred_lists p;
	p.first.assign(n + 1, 0);
	for (uint32_t i = 0; i < n; i++)
		if (out.annot[i].reached)
			for (const edge s : succs(out, i))
				p.first[s.to + 1]++;
	for (size_t i = 0; i < n; i++)
		p.first[i + 1] += p.first[i];
	p.list.resize(p.first[n]);
	std::vector<uint32_t> at(p.first.begin(), p.first.end() - 1);
	for (uint32_t i = 0; i < n; i++)
		if (out.annot[i].reached)
			for (const edge s : succs(out, i))
				p.list[at[s.to]++] = i;
	return p;
}

} // namespace xlate
