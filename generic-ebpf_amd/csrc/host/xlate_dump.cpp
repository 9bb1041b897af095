// xlate_dump.cpp — EBPF_XLATE_DUMP=file: the translation as translate_program leaves it, written
// once when it returns, on success and on failure (tools/translation_digest.py hashes it).
//
//   err <errno> <message>
//   start <entry>
//   one line per scalar and per list field of dprog_host (those the lowering sets included;
//   translate_ms, a time, left out)
//   <index> kind .. aux ..   one line per entry; a reached entry's line ends in its in[]: one
//                            kind:map:off per register (off in hex: a constant may be a handle)
//
// Depends on nothing of the translator but dprog_host, so the same file serves any tree.
#include "internal.h"

void
xlate_dump(const dprog_host &out, int err)
{
	const char *path = getenv("EBPF_XLATE_DUMP");
	FILE *f = path != nullptr ? fopen(path, "w") : nullptr;
	if (f == nullptr)
		return;
	fprintf(f, "err %d %s\n", err, out.error_msg.c_str());
	fprintf(f, "start %u\n", out.start);
	const std::pair<const char *, unsigned long long> scalars[] = {
	    {"error", (unsigned long long)out.error}, {"writes_memory", out.writes_memory},
	    {"asm_needs_general", out.asm_needs_general}, {"asm_gstage", out.asm_gstage},
	    {"asm_pktv", out.asm_pktv}, {"asm_hdrlds", out.asm_hdrlds}, {"asm_keep", out.asm_keep},
	    {"max_stack", out.max_stack}, {"max_updates", out.max_updates}, {"has_loops", out.has_loops},
	    {"vstore_sites", out.vstore_sites}, {"vstore_overlay", out.vstore_overlay},
	    {"ovl_entries", out.ovl_entries}, {"write_cap", out.write_cap},
	    {"reads_counters", out.reads_counters}};
	for (const auto &s : scalars)
		fprintf(f, "%s %llu\n", s.first, s.second);
	fprintf(f, "maps");
	for (const struct ebpf_map *m : out.maps)
		fprintf(f, " %#llx", (unsigned long long)(uintptr_t)m);
	fprintf(f, "\n");
	auto list = [&](const char *name, const auto &v) {
		fprintf(f, "%s", name);
		for (auto x : v)
			fprintf(f, " %u", (unsigned)x);
		fprintf(f, "\n");
	};
	list("upd_maps", out.upd_maps);
	list("vstore_maps", out.vstore_maps);
	list("hupd_maps", out.hupd_maps);
	list("atomic_maps", out.atomic_maps);
	list("atomic_width", out.atomic_width);
	fprintf(f, "entries %zu annot %zu\n", out.entries.size(), out.annot.size());
	for (size_t i = 0; i < out.entries.size(); i++) {
		const dp_entry &e = out.entries[i];
		fprintf(f, "%zu kind %#x dst %u src %u off %d imm %#llx next %u target %u aux %#x", i, e.kind,
			e.dst, e.src, e.off, (unsigned long long)e.imm, e.next, e.target, e.aux);
		if (i < out.annot.size() && out.annot[i].reached) {
			fprintf(f, " in");
			for (const av &a : out.annot[i].in)
				fprintf(f, " %u:%d:%#llx", a.kind, a.map, (unsigned long long)a.off);
		}
		fprintf(f, "\n");
	}
	fclose(f);
}
