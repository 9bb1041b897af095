// wants_values.h — shared by reduce.h and rollup.h, and so by the host runtime and the launchers.
#pragma once

// Does an output read the values?  (ebpf_batch_sums, ebpf_batch_rolls: sum, min, max or bits.)
template <typename O>
inline bool
wants_values(const O &out)
{
	return out.sum != nullptr || out.min != nullptr || out.max != nullptr || out.bits != nullptr;
}
