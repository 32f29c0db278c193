// rsqc_umi.h -- the UMI key of --umi-tag / --umi-qname (rsqc_batch.umi, rsqc_umi_pack), written once as __host__ __device__
// code like rsqc_bamrec.h: the device decode kernels, the host reader and the emulation harnesses run this one definition.
//
//   A C G T (either case)   bases, 2 bits each, the first base most significant
//   - and +                 the joiners of dual UMIs: skipped
//   key                     (1 << 2L) | bits for L bases -- the length is part of the key, no usable UMI packs to 0
//   0 = "no usable UMI"     nothing left after the joiners, any other byte (N included), more than 31 bases
// The key is exact, not a hash: two different usable UMIs never share one.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RSQC_UMI_FN __host__ __device__ __forceinline__
#else
#define RSQC_UMI_FN inline
#endif

#define RSQC_UMI_MAX_BASES 31u
#define RSQC_UMI_NONE 0u           /* BamTagSpec.umi_src: no source selected */
#define RSQC_UMI_TAG 1u            /* the first aux field umi_t0 umi_t1 of type Z */
#define RSQC_UMI_QNAME 2u          /* the bytes of QNAME behind the last umi_sep */

namespace rsqc {

RSQC_UMI_FN uint64_t umi_pack(const uint8_t *s, uint32_t len) {
    uint64_t bits = 0; uint32_t n = 0;
    for (uint32_t i = 0; i < len; ++i) {
        const uint32_t b = s[i];
        if (b == '-' || b == '+') continue;
        uint32_t code;
        switch (b | 0x20u) {                          // (only the letter's two cases give its lower case with this bit set)
        case 'a': code = 0; break;
        case 'c': code = 1; break;
        case 'g': code = 2; break;
        case 't': code = 3; break;
        default: return 0;
        }
        if (++n > RSQC_UMI_MAX_BASES) return 0;
        bits = (bits << 2) | code;
    }
    return n ? ((1ull << (2u * n)) | bits) : 0ull;
}

// the UMI of a read name: the bytes behind the last `sep`; no separator, or nothing behind it, is no UMI
RSQC_UMI_FN uint64_t umi_from_qname(const uint8_t *name, uint32_t len, uint8_t sep) {
    for (uint32_t i = len; i > 0; --i)
        if (name[i - 1] == sep) return umi_pack(name + i, len - i);
    return 0;
}

}  // namespace rsqc
