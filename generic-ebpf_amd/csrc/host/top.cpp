// top.cpp — the heaviest entries (ebpf_gpu.h "The heaviest entries"): the k best entries of a keyed
// sequence by a bit field of the value, on the host (ebpf_batch_top, the statement of the
// semantics) and on the device (ebpf_batch_top_dev, top.hip).
#include "top.h"
#include "list_args.h"

#include <numeric>
#include <vector>

namespace {

int
top_args(const uint64_t *keys, const uint64_t *vals, uint64_t cap, uint32_t flags, uint32_t val_shift,
	 uint32_t val_bits, uint64_t k, const struct ebpf_batch_tops *out, const uint64_t *info)
{
	if (out == nullptr || info == nullptr)
		return fail(EINVAL, "out or info is NULL");
	if (flags & ~(EBPF_TOP_SMALLEST | EBPF_TOP_SEGMENTS))
		return fail(EINVAL, "unknown flags");
	if (int err = check_field(val_shift, val_bits))
		return err;
	if (cap != 0 && vals == nullptr)
		return fail(EINVAL, "vals is NULL with cap > 0");
	if (out->keys != nullptr && keys == nullptr)
		return fail(EINVAL, "out->keys is wanted and keys is NULL");
	if (cap > 0xffffffffull || k > EBPF_TOP_MAX)
		return fail(E2BIG, "cap above 2^32 - 1 or k above EBPF_TOP_MAX");
	return 0;
}

} // namespace

// A partial sort over positions: the reference for the device kernels.
EBPF_EXPORT int
ebpf_batch_top(const uint64_t *keys, const uint64_t *vals, uint64_t cap, const uint64_t *n,
	       uint32_t flags, uint32_t val_shift, uint32_t val_bits, uint64_t k,
	       const struct ebpf_batch_tops *out, uint64_t *info)
{
	if (int err = top_args(keys, vals, cap, flags, val_shift, val_bits, k, out, info))
		return err;
	const uint64_t N = entry_count(n, cap, flags & EBPF_TOP_SEGMENTS), m = k < N ? k : N;
	const bit_field f = field_of(val_shift, val_bits);
	const bool smallest = flags & EBPF_TOP_SMALLEST;
	std::vector<uint32_t> p(N);
	std::iota(p.begin(), p.end(), 0u);
	std::partial_sort(p.begin(), p.begin() + m, p.end(), [&](uint32_t a, uint32_t b) {
		const uint64_t fa = f.of(vals[a]), fb = f.of(vals[b]);
		return fa != fb ? (smallest ? fa < fb : fa > fb) : a < b;
	});
	for (uint64_t j = 0; j < m; j++) {
		if (out->keys != nullptr)
			out->keys[j] = keys[p[j]];
		if (out->vals != nullptr)
			out->vals[j] = vals[p[j]];
		if (out->pos != nullptr)
			out->pos[j] = p[j];
	}
	const uint64_t cut = m != 0 ? f.of(vals[p[m - 1]]) : 0;
	uint64_t ties = 0;
	for (uint64_t j = m; m != 0 && j < N; j++)
		ties += f.of(vals[p[j]]) == cut ? 1 : 0;
	info[0] = m;
	info[1] = N;
	info[2] = cut;
	info[3] = ties;
	return 0;
}

EBPF_EXPORT int
ebpf_batch_top_dev(int device, const uint64_t *keys_dev, const uint64_t *vals_dev, uint64_t cap,
		   const uint64_t *n_dev, uint32_t flags, uint32_t val_shift, uint32_t val_bits,
		   uint64_t k, const struct ebpf_batch_tops *out, uint64_t *info_dev, void *stream)
{
	int err = top_args(keys_dev, vals_dev, cap, flags, val_shift, val_bits, k, out, info_dev);
	if (err || (err = check_device(device)))
		return err;
	return on_device(device, stream, top_scratch_bytes(cap), "top kernels",
			 [&](hipStream_t st, uint32_t *scratch) {
		return launch_top(keys_dev, vals_dev, cap, n_dev, flags, val_shift, val_bits, k, *out,
				  info_dev, scratch, st);
	});
}
