// rollup.cpp — rolling a table up (ebpf_gpu.h "Rolling a table up"): the runs of equal key prefix
// of a keyed sequence reduced, on the host (ebpf_batch_rollup, the statement of the semantics) and
// on the device (ebpf_batch_rollup_dev, rollup.hip).
#include "rollup.h"
#include "list_args.h"

namespace {

int
rollup_args(const uint64_t *keys, const uint64_t *vals, uint64_t cap, uint32_t flags,
	    uint32_t key_shift, uint32_t val_shift, uint32_t val_bits, uint64_t out_cap,
	    const struct ebpf_batch_rolls *out, const uint64_t *info)
{
	if (out == nullptr || info == nullptr)
		return fail(EINVAL, "out or info is NULL");
	if (flags & ~EBPF_ROLLUP_SEGMENTS)
		return fail(EINVAL, "unknown flags");
	if (key_shift > 63)
		return fail(EINVAL, "key_shift above 63");
	if (wants_values(*out))
		if (int err = check_field(val_shift, val_bits))
			return err;
	if (cap != 0 && keys == nullptr)
		return fail(EINVAL, "keys is NULL with cap > 0");
	if (cap != 0 && vals == nullptr && wants_values(*out))
		return fail(EINVAL, "vals is NULL with cap > 0 and an output of the values wanted");
	if (cap > 0xffffffffull || out_cap > 0xffffffffull)
		return fail(E2BIG, "cap or out_cap above 2^32 - 1");
	return 0;
}

} // namespace

// One pass over the entries: the reference for the device kernels.
EBPF_EXPORT int
ebpf_batch_rollup(const uint64_t *keys, const uint64_t *vals, uint64_t cap, const uint64_t *n,
		  uint32_t flags, uint32_t key_shift, uint32_t val_shift, uint32_t val_bits,
		  uint64_t out_cap, const struct ebpf_batch_rolls *out, uint64_t *info)
{
	if (int err = rollup_args(keys, vals, cap, flags, key_shift, val_shift, val_bits, out_cap, out,
				  info))
		return err;
	const uint64_t N = entry_count(n, cap, flags & EBPF_ROLLUP_SEGMENTS);
	const bool values = wants_values(*out);
	const bit_field f = values ? field_of(val_shift, val_bits) : field_of(0, 64);
	uint64_t C = 0;
	for (uint64_t a = 0, b; a < N; a = b, C++) {
		const uint64_t c = keys[a] >> key_shift;
		uint64_t sum = 0, mn = ~0ull, mx = 0, bits = 0;
		for (b = a; b < N && keys[b] >> key_shift == c; b++) {
			if (!values)
				continue;
			const uint64_t v = f.of(vals[b]);
			sum += v;
			mn = v < mn ? v : mn;
			mx = v > mx ? v : mx;
			bits |= v;
		}
		if (C >= out_cap)
			continue;
		if (out->keys != nullptr)
			out->keys[C] = c;
		if (out->count != nullptr)
			out->count[C] = b - a;
		if (out->sum != nullptr)
			out->sum[C] = sum;
		if (out->min != nullptr)
			out->min[C] = mn;
		if (out->max != nullptr)
			out->max[C] = mx;
		if (out->bits != nullptr)
			out->bits[C] = bits;
		if (out->starts != nullptr)
			out->starts[C] = a;
	}
	if (out->starts != nullptr && C <= out_cap)
		out->starts[C] = N;
	info[0] = C;
	info[1] = N;
	if (C > out_cap)
		return fail(ENOSPC, "more runs than out_cap");
	return 0;
}

EBPF_EXPORT int
ebpf_batch_rollup_dev(int device, const uint64_t *keys_dev, const uint64_t *vals_dev, uint64_t cap,
		      const uint64_t *n_dev, uint32_t flags, uint32_t key_shift, uint32_t val_shift,
		      uint32_t val_bits, uint64_t out_cap, const struct ebpf_batch_rolls *out,
		      uint64_t *info_dev, void *stream)
{
	int err = rollup_args(keys_dev, vals_dev, cap, flags, key_shift, val_shift, val_bits, out_cap,
			      out, info_dev);
	if (err || (err = check_device(device)))
		return err;
	return on_device(device, stream, rollup_scratch_bytes(cap), "rollup kernels",
			 [&](hipStream_t st, uint32_t *scratch) {
		return launch_rollup(keys_dev, vals_dev, cap, n_dev, flags, key_shift, val_shift, val_bits,
				     out_cap, *out, info_dev, reinterpret_cast<uint64_t *>(scratch), st);
	});
}
