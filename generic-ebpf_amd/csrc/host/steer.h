// steer.h — shared by steer.cpp and steer.hip (ebpf_batch_steer_dev, ebpf_batch_select_dev: a
// batch's packets grouped by verdict class on the device).  STEER_TILE is every list kernel's tile
// (hip/wave_rank.h: steer, group; hip/seg_tile.h: reduce, scan, filter); group.hip shares the scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ebpf_pkt_batch;

// Packets per tile: one workgroup of 256 counts, and later ranks, STEER_TILE consecutive packets
// (each of its four waves a contiguous quarter).  native.py STEER_TILE repeats the number.
constexpr uint32_t STEER_TILE = 4096;
// Past this many tiles the tile scan takes two levels (segments of tiles, then the tiles of each).
constexpr uint32_t STEER_SEGS = 256;

// Scratch of one steering call, in u32 words: a row of EBPF_HIST_BINS per tile, (two levels) per
// segment, and one of class totals.  Any contents on entry.
size_t steer_scratch_words(uint64_t count);
// The tile scan on its own (group.hip's radix passes share it): scratch holds ntiles rows of class
// counts, laid out as above.  Leaves starts[b] = the packets of the classes below b, for b in
// [0, EBPF_HIST_BINS], and rows[t][b] = the packets of class b in the tiles before t, plus
// starts[b] already iff it returns true (more than STEER_SEGS tiles).
bool launch_tile_scan(uint32_t *scratch, uint32_t ntiles, uint64_t *starts, hipStream_t stream);
// index[starts[b] .. starts[b+1]) = the packets of class b in ascending order (count >= 1,
// count <= 0xffffffff); faults may be NULL.
hipError_t launch_steer(const uint64_t *ret, const uint8_t *faults, uint64_t count, uint32_t *index,
			uint64_t *starts, uint32_t *scratch, hipStream_t stream);
// extents[2j], extents[2j+1] = (start, end) of packet index[j] of `b` (device pointers), or (0, 0)
// for an index >= b.count; n >= 1.
hipError_t launch_select(const struct ebpf_pkt_batch &b, const uint32_t *index, uint64_t n,
			 uint64_t *extents, hipStream_t stream);
