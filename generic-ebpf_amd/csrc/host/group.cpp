// group.cpp — grouping a batch by a wide verdict key (ebpf_gpu.h "Grouping a batch by key"): the
// packets sorted stably by a bit field of ret, and the table of the groups of equal keys, on the
// host (ebpf_batch_group) and on the device (ebpf_batch_group_dev).
#include <numeric>
#include <vector>

#include "group.h"
#include "list_args.h"
#include "steer.h"

namespace {

int
group_args(const uint64_t *ret, uint64_t count, uint32_t key_shift, uint32_t key_bits,
	   const uint32_t *index, uint64_t group_cap, const uint64_t *group_starts, const uint64_t *info)
{
	if (int err = check_field(key_shift, key_bits, "key"))
		return err;
	if (info == nullptr || (count != 0 && (ret == nullptr || index == nullptr)))
		return fail(EINVAL, "ret, index or info is NULL");
	if (group_cap != 0 && group_starts == nullptr)
		return fail(EINVAL, "group_starts is NULL with group_cap > 0");
	if (count > 0xffffffffull)
		return fail(E2BIG, "count above 2^32 - 1: the packet index is 32 bits");
	return 0;
}

} // namespace

group_plan
group_plan_of(uint32_t key_bits)
{
	const uint32_t passes = (key_bits + 7) / 8;
	return {passes, (key_bits + passes - 1) / passes, key_bits <= 32 ? 4u : 8u};
}

size_t
group_tmp_bytes(uint64_t count, uint32_t key_bits)
{
	const group_plan plan = group_plan_of(key_bits);
	const uint64_t per = plan.passes > 1 ? 2 * plan.key_bytes + 4 : plan.key_bytes;
	return (size_t)(group_padded(count) * per);
}

EBPF_EXPORT size_t
ebpf_batch_group_tmp_bytes(uint64_t count, uint32_t key_bits)
{
	if (!field_ok(0, key_bits) || count > 0xffffffffull)
		return 0;
	return group_tmp_bytes(count, key_bits);
}

// A stable sort on (faulted, key): the reference for the device kernels.
EBPF_EXPORT int
ebpf_batch_group(const uint64_t *ret, const uint8_t *faults, uint64_t count, uint32_t key_shift,
		 uint32_t key_bits, uint32_t *index, uint64_t group_cap, uint64_t *group_keys,
		 uint64_t *group_starts, uint64_t *info)
{
	int err = group_args(ret, count, key_shift, key_bits, index, group_cap, group_starts, info);
	if (err)
		return err;
	const bit_field kf = field_of(key_shift, key_bits);
	auto key = [&](uint32_t i) { return kf.of(ret[i]); };
	auto faulted = [&](uint32_t i) { return faults != nullptr && faults[i] != 0; };
	std::vector<uint32_t> order((size_t)count);
	std::iota(order.begin(), order.end(), 0u);
	std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
		if (faulted(a) || faulted(b))
			return !faulted(a) && faulted(b);
		return key(a) < key(b);
	});
	uint64_t unfaulted = 0, groups = 0;
	for (uint64_t p = 0; p < count; p++) {
		index[p] = order[p];
		if (faulted(order[p]))
			continue;
		unfaulted++;
		if (p != 0 && key(order[p - 1]) == key(order[p]))
			continue;
		if (groups < group_cap) {
			group_starts[groups] = p;
			if (group_keys != nullptr)
				group_keys[groups] = key(order[p]);
		}
		groups++;
	}
	info[0] = groups;
	info[1] = unfaulted;
	if (groups > group_cap)
		return fail(ENOSPC, "more groups than group_cap");
	if (group_starts != nullptr)
		group_starts[groups] = unfaulted;
	return 0;
}

EBPF_EXPORT int
ebpf_batch_group_dev(int device, const uint64_t *ret_dev, const uint8_t *faults_dev, uint64_t count,
		     uint32_t key_shift, uint32_t key_bits, uint32_t *index_dev, uint64_t group_cap,
		     uint64_t *group_keys_dev, uint64_t *group_starts_dev, uint64_t *info_dev,
		     void *tmp_dev, size_t tmp_bytes, void *stream)
{
	int err = group_args(ret_dev, count, key_shift, key_bits, index_dev, group_cap, group_starts_dev,
			     info_dev);
	if (err)
		return err;
	const size_t need = group_tmp_bytes(count, key_bits);
	if (tmp_bytes < need)
		return fail(ENOSPC, "tmp_bytes below ebpf_batch_group_tmp_bytes(count, key_bits)");
	if (need != 0 && tmp_dev == nullptr)
		return fail(EINVAL, "tmp_dev is NULL");
	if ((err = check_device(device)))
		return err;
	return on_device(device, stream, count != 0 ? group_scratch_words(count) * sizeof(uint32_t) : 0,
			 count != 0 ? "grouping kernels" : "hipMemsetAsync(info)",
			 [&](hipStream_t st, uint32_t *scratch) {
		if (count == 0) {
			hipError_t e = hipMemsetAsync(info_dev, 0, 2 * sizeof(uint64_t), st);
			if (e == hipSuccess && group_starts_dev != nullptr)
				e = hipMemsetAsync(group_starts_dev, 0, sizeof(uint64_t), st);
			return e;
		}
		return launch_group(ret_dev, faults_dev, count, key_shift, key_bits, index_dev, group_cap,
				    group_keys_dev, group_starts_dev, info_dev, tmp_dev, scratch, st);
	});
}
