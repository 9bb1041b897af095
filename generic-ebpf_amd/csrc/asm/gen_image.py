"""The build knobs (EBPF_ASM_* environment variables, read here and nowhere else) and the table of
the three images the generator writes.  An Image says everything that makes one image's code
differ from another's; every function whose output depends on the image takes it as its first
argument."""
import os
from typing import NamedTuple

from gen_abi import GEN_JOIN, NSGPR_GEN, NSGPR_INTERP, NSGPR_STAGED


class Settings(NamedTuple):
    st_policy: str        # cache-policy suffix of the result stores
    ld_policy: str        # ... of the packet DMA loads
    probe_policy: str     # ... of the hashtable probe loads
    retk: int             # result groups per burst of the staged image m1
    gen_hoist_regs: int   # general image: spare VGPRs for hoisted packet loads


def read_settings(env):
    # cache policy of the streaming accesses (EBPF_ASM_NT bit 0 = ret stores nt, bit 1 = packet DMA
    # loads nt).  Both nt by default: the once-read packet stream with nt DMA reads 6.75 TB/s against
    # 6.06 TB/s default policy (tools/ubench/floor.hip, profiles/r01/ubench/)
    nt = int(env.get("EBPF_ASM_NT", "3"))

    def policy(var, default):
        # explicit cache-policy strings (A/B probes of the gfx950 sc0/sc1/nt bits), "+"-separated,
        # e.g. EBPF_ASM_LDPOL=sc1+nt ("none" = no bits)
        if not env.get(var):
            return default
        p = env[var].replace("+", " ")
        return "" if p == "none" else " " + p

    # Results of RETK consecutive groups are kept in VGPRs and written as one RETK x 512-B burst
    # (RETK > 1 adds 2*RETK VGPRs at v64).  Each wave walks superblocks of RETK consecutive groups.
    # Default 8: one aligned 4-KB result burst per wave reads+writes at 5.6-5.7 TB/s against
    # 5.1 TB/s for 512-B stores (floor.hip), worth the 6 instead of 8 waves per SIMD it costs.
    retk = int(env.get("EBPF_ASM_RETK", "8"))
    assert retk in (1, 2, 4, 8)
    return Settings(
        st_policy=policy("EBPF_ASM_STPOL", " nt" if nt & 1 else ""),
        ld_policy=policy("EBPF_ASM_LDPOL", " nt" if nt & 2 else ""),
        # hashtable probe loads (A/B: EBPF_ASM_PROBEPOL, same form; default policy)
        probe_policy=policy("EBPF_ASM_PROBEPOL", ""),
        retk=retk,
        # general image: spare VGPRs v64.. for packet loads the code generator issues ahead
        # (asm_cc.cpp hoist plan); 16 cost the general kernels 8 -> 6 waves per SIMD
        gen_hoist_regs=int(env.get("EBPF_ASM_GENHOIST", "16")))


SETTINGS = read_settings(os.environ)


class Image(NamedTuple):
    name: str
    staged: bool          # staged (fixed 64-B packets) or general kernels
    interp: bool          # the image the assembly interpreter launches from
    retk: int             # result groups per burst

    @property
    def v_rb(self):
        """First VGPR of the result slots: v[44:45] itself (one group) or v64.."""
        return 44 if self.retk == 1 else 64

    @property
    def slots(self):
        """Result slots: retk, and 16 in the staged image with result bursts, whose wide kernel
        (ebpf_jit_s64w) allocates the second 8 for write phasing (store_phased)."""
        return 16 if self.retk == 8 else self.retk

    @property
    def nvgpr(self):
        n = 64 if self.retk == 1 else 64 + 2 * self.retk
        return n if self.staged else n + SETTINGS.gen_hoist_regs

    @property
    def nvgpr_wide(self):
        """The wide kernel's VGPRs (0: the image has none)."""
        return self.v_rb + 2 * self.slots if self.staged and self.slots == 16 else 0

    @property
    def phased(self):
        """The image's kernels keep result slots that store_phased can write."""
        return self.staged and self.retk > 1

    @property
    def nsgpr(self):
        return NSGPR_STAGED if (self.staged or GEN_JOIN) else NSGPR_GEN

    @property
    def nsgpr_interp(self):
        """... of ebpf_interp_s64: see NSGPR_INTERP."""
        return NSGPR_INTERP if self.interp else self.nsgpr


# Three code objects: the staged (fixed 64-B) kernels use EBPF_ASM_RETK; the general kernels (any
# stride / offsets: latency-bound per-packet loads, where the 8 waves per SIMD of one result
# group matter more than the store burst) and the interpreter's staged image (NSGPR_INTERP: it
# is bound by resident waves) keep one result group per burst.
IMAGES = (Image("m1", staged=True, interp=False, retk=SETTINGS.retk),
          Image("m0", staged=False, interp=False, retk=1),
          Image("m3", staged=True, interp=True, retk=1))
