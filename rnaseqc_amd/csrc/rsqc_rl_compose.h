// rsqc_rl_compose.h -- "Read Length" (src/RNASeQC.cpp:275-278) of a whole file from the per-batch / per-range transfer functions
// (rsqc_shard_info; the tables read_length_kernel of rsqc_kr.h leaves).  Plain host C++, no HIP: included by rsqc_finalize.cpp (a pass
// that held batches of several file ranges), by host/main.cpp (the merge of a --gpus run's shards) and, unmodified, by the emulation
// of the tests (tests/hostemu/k1_emu.cpp), so that all three apply the tables with the same loop -- and the text of the
// one error this stage can raise (rsqc_submit.cpp: device_error_message).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace rsqc {

struct RlTable { uint64_t file_index; const uint32_t *span; const int32_t *state; uint32_t n; };   // one batch or range: n (key, state) pairs, keys ascending

// one table applied to the state r: the first key above the state decides, no such key leaves it (rsqc_kr.h)
inline uint32_t rl_apply(const RlTable &t, uint32_t r) {
    for (uint32_t k = 0; k < t.n; ++k)
        if (t.span[k] > r) return (uint32_t)t.state[k];
    return r;
}

// the tables of all batches / ranges (of all shards) in ascending file index, from state 0; `tables` is reordered
inline int32_t rl_compose(std::vector<RlTable> &tables) {
    std::stable_sort(tables.begin(), tables.end(), [](const RlTable &a, const RlTable &b) { return a.file_index < b.file_index; });
    uint32_t r = 0;
    for (const RlTable &t : tables) r = rl_apply(t, r);
    return (int32_t)r;
}

// The message of a pass that ended on the limit of 128 prefix maxima per batch or file range (RSQC_RL_MAXP, rsqc_kr.h): the kernel sets
// bit 0 of the flag word of the offender's summary slot.  flags[k * stride] = the flag word of entry k of n; empty when no entry is flagged.
inline std::string rl_limit_message(const uint32_t *flags, size_t stride, size_t n, const uint64_t *file_index, const uint64_t *records) {
    for (size_t k = 0; k < n; ++k)
        if (flags[k * stride] & 1u)
            return "Read Length: the batch or file range at file index " + std::to_string(file_index[k]) + " (" + std::to_string(records[k]) +
                   " records) holds more than 128 prefix maxima of the alignment span among reads of differing length; the limit of one batch or"
                   " range is 128 (hand these records over in smaller batches or ranges)";
    return std::string();
}

}  // namespace rsqc
