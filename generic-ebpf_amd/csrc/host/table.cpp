// table.cpp — carrying totals across batches (ebpf_gpu.h "Carrying totals across batches"): a
// sorted table of keys and values, looked up and merged into on the host (ebpf_batch_lookup,
// ebpf_batch_accumulate, the statement of the semantics) and on the device (the _dev functions,
// table.hip).
#include "table.h"
#include "list_args.h"

namespace {

const struct ebpf_key_table NO_TABLE = {nullptr, nullptr, 0, nullptr};

int
table_null(const struct ebpf_key_table &t)
{
	if (t.cap != 0 && (t.keys == nullptr || t.vals == nullptr || t.n == nullptr))
		return fail(EINVAL, "keys, vals or n of a table with cap > 0 is NULL");
	return 0;
}

int
lookup_args(const struct ebpf_key_table *table, const uint64_t *keys, uint64_t key_cap, uint32_t mode)
{
	if (table == nullptr)
		return fail(EINVAL, "table is NULL");
	if (mode != EBPF_LOOKUP_VALUE && mode != EBPF_LOOKUP_REMAINING)
		return fail(EINVAL, "unknown mode");
	if (key_cap != 0 && keys == nullptr)
		return fail(EINVAL, "keys is NULL with key_cap > 0");
	if (int err = table_null(*table))
		return err;
	if (key_cap > 0xffffffffull || table->cap > 0xffffffffull)
		return fail(E2BIG, "key_cap or the table's cap above 2^32 - 1");
	return 0;
}

int
accumulate_args(const struct ebpf_key_table *in, const uint64_t *keys, const uint64_t *adds,
		uint64_t key_cap, uint32_t op, const struct ebpf_key_table *out, const uint64_t *info)
{
	if (out == nullptr || info == nullptr)
		return fail(EINVAL, "out or info is NULL");
	if (op > EBPF_ACC_OR)
		return fail(EINVAL, "unknown op");
	if (key_cap != 0 && (keys == nullptr || adds == nullptr))
		return fail(EINVAL, "keys or adds is NULL with key_cap > 0");
	int err = in != nullptr ? table_null(*in) : 0;
	if (err || (err = table_null(*out)))
		return err;
	if (key_cap > 0xffffffffull || (in != nullptr && in->cap > 0xffffffffull) ||
	    out->cap > 0xffffffffull)
		return fail(E2BIG, "key_cap or a table's cap above 2^32 - 1");
	return 0;
}

// The valid entries of a table (one without n has cap 0, by table_null: no entry).
uint64_t
entries(const struct ebpf_key_table &t)
{
	return entry_count(t.n, t.cap, false);
}

int
check_ascending(const uint64_t *keys, uint64_t m, const char *what)
{
	for (uint64_t p = 1; p < m; p++)
		if (keys[p - 1] >= keys[p])
			return fail(EINVAL, std::string(what) + " is not strictly ascending");
	return 0;
}

uint64_t
combine(uint32_t op, uint64_t a, uint64_t b)
{
	switch (op) {
	case EBPF_ACC_ADD:
		return a + b;
	case EBPF_ACC_MIN:
		return a < b ? a : b;
	case EBPF_ACC_MAX:
		return a > b ? a : b;
	default:
		return a | b;
	}
}

} // namespace

// A binary search per key: the reference for the device kernel.
EBPF_EXPORT int
ebpf_batch_lookup(const struct ebpf_key_table *table, const uint64_t *keys, uint64_t key_cap,
		  const uint64_t *nkeys, uint32_t mode, uint64_t missing, uint64_t limit,
		  uint64_t *vals_out, uint32_t *pos_out)
{
	int err = lookup_args(table, keys, key_cap, mode);
	if (err)
		return err;
	const uint64_t N = entries(*table), R = seg_count(nkeys, key_cap);
	if ((err = check_ascending(table->keys, N, "the table")))
		return err;
	for (uint64_t g = 0; g < R; g++) {
		const uint64_t p = std::lower_bound(table->keys, table->keys + N, keys[g]) - table->keys;
		const bool there = p < N && table->keys[p] == keys[g];
		const uint64_t v = there ? table->vals[p] : missing;
		if (pos_out != nullptr)
			pos_out[g] = there ? (uint32_t)p : EBPF_NO_ENTRY;
		if (vals_out != nullptr)
			vals_out[g] = mode == EBPF_LOOKUP_VALUE ? v : (v < limit ? limit - v : 0);
	}
	return 0;
}

// One merge of the two sorted sequences: the reference for the device kernels.
EBPF_EXPORT int
ebpf_batch_accumulate(const struct ebpf_key_table *in, const uint64_t *keys, const uint64_t *adds,
		      uint64_t key_cap, const uint64_t *nkeys, uint32_t op, uint64_t keep_lo,
		      uint64_t keep_hi, const struct ebpf_key_table *out, uint64_t *info)
{
	int err = accumulate_args(in, keys, adds, key_cap, op, out, info);
	if (err)
		return err;
	const struct ebpf_key_table &t = in != nullptr ? *in : NO_TABLE;
	const uint64_t N = entries(t), R = seg_count(nkeys, key_cap);
	if ((err = check_ascending(t.keys, N, "the table")) || (err = check_ascending(keys, R, "keys")))
		return err;
	uint64_t M = 0, fresh = 0, left_out = 0;
	for (uint64_t p = 0, g = 0; p < N || g < R;) {
		// the next candidate: the smaller of the two heads, or both where they are equal
		const bool from_table = p < N && (g == R || t.keys[p] <= keys[g]);
		const bool from_batch = g < R && (p == N || keys[g] <= t.keys[p]);
		const uint64_t key = from_table ? t.keys[p] : keys[g];
		const uint64_t v = from_table && from_batch ? combine(op, t.vals[p], adds[g])
							    : (from_table ? t.vals[p] : adds[g]);
		p += from_table ? 1 : 0;
		g += from_batch ? 1 : 0;
		if (v < keep_lo || v > keep_hi) {
			left_out++;
			continue;
		}
		if (M < out->cap) {
			out->keys[M] = key;
			out->vals[M] = v;
		}
		M++;
		fresh += from_table ? 0 : 1;
	}
	if (out->n != nullptr)
		*out->n = M;
	info[0] = M;
	info[1] = fresh;
	info[2] = left_out;
	return M > out->cap ? fail(ENOSPC, "the output table is short") : 0;
}

EBPF_EXPORT int
ebpf_batch_lookup_dev(int device, const struct ebpf_key_table *table, const uint64_t *keys_dev,
		      uint64_t key_cap, const uint64_t *nkeys_dev, uint32_t mode, uint64_t missing,
		      uint64_t limit, uint64_t *vals_out_dev, uint32_t *pos_out_dev, void *stream)
{
	int err = lookup_args(table, keys_dev, key_cap, mode);
	if (err || (err = check_device(device)))
		return err;
	if (vals_out_dev == nullptr && pos_out_dev == nullptr)
		return 0;
	return on_device(device, stream, 0, "lookup kernel", [&](hipStream_t st, uint32_t *) {
		return launch_lookup(*table, keys_dev, key_cap, nkeys_dev, mode, missing, limit,
				     vals_out_dev, pos_out_dev, st);
	});
}

EBPF_EXPORT int
ebpf_batch_accumulate_dev(int device, const struct ebpf_key_table *in, const uint64_t *keys_dev,
			  const uint64_t *adds_dev, uint64_t key_cap, const uint64_t *nkeys_dev,
			  uint32_t op, uint64_t keep_lo, uint64_t keep_hi,
			  const struct ebpf_key_table *out, uint64_t *info_dev, void *stream)
{
	int err = accumulate_args(in, keys_dev, adds_dev, key_cap, op, out, info_dev);
	if (err || (err = check_device(device)))
		return err;
	const struct ebpf_key_table &t = in != nullptr ? *in : NO_TABLE;
	return on_device(device, stream, accumulate_scratch_bytes(t.cap, key_cap), "accumulate kernels",
			 [&](hipStream_t st, uint32_t *scratch) {
		return launch_accumulate(t, keys_dev, adds_dev, key_cap, nkeys_dev, op, keep_lo, keep_hi,
					 *out, info_dev, scratch, st);
	});
}
