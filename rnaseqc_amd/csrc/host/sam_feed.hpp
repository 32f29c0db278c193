// sam_feed.hpp -- SAM input for the command line: the format of an input file by its content (BAM, BGZF-compressed SAM, SAM
// text), the SAM header's @SQ lines, and the feeder of plain SAM text for the device SAM stages (rsqc_decode_submit_text).
// The reference opens all three through htslib's hts_open (src/BamReader.h, SeqLib); CRAM and plain (non-BGZF) gzip are
// not read here.
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace rsqc_host {

enum class InputFormat { Unopenable = -1, PlainGzip = -2, Unknown = 0, SamText = 1, SamBgzf = 2, Bam = 3 };
const char *input_format_name(InputFormat f);

// the format of the bytes that start a file: BGZF whose first inflated bytes are "BAM\1" -> Bam, other BGZF -> SamBgzf,
// gzip that is not BGZF -> PlainGzip, anything else -> SamText (the SAM parse judges it)
InputFormat sniff_format(const uint8_t *head, size_t n);
InputFormat sniff_file(const std::string &path);            // a regular file (pread of its first block)

struct SamHeader {
    std::vector<std::string> names;                          // @SQ SN:, in order
    std::vector<uint64_t> lengths;                           // @SQ LN: (0 when absent)
    uint64_t lines = 0;                                      // header lines
};
// the '@' lines at the start of `text` (complete = false: the header may go on behind the bytes given)
void parse_sam_header(const char *text, size_t n, SamHeader &h, bool &complete);
// the header of a SAM text or BGZF SAM file (gzread reads both); false = unreadable
bool read_sam_header(const std::string &path, SamHeader &h);

// Plain SAM text in page-locked chunks, read sequentially (read(2): a FIFO or /dev/stdin works) by a read-ahead thread.
class SamTextFeeder {
public:
    struct Chunk { uint8_t *data = nullptr; size_t cap = 0, bytes = 0, alloc = 0; bool pinned = false; };   // cap: bytes a chunk holds for this file; alloc: allocated
    SamTextFeeder() = default;
    ~SamTextFeeder();
    SamTextFeeder(const SamTextFeeder &) = delete;
    SamTextFeeder &operator=(const SamTextFeeder &) = delete;
    bool open(const std::string &path);                      // may be called again for the next file: the chunk buffers are kept
    // the first bytes of the input (read and kept: they are the first chunk's); sniffs a stream without losing them
    const std::vector<uint8_t> &peek(size_t n);
    void start(size_t chunk_bytes);
    Chunk *next();                                           // nullptr at the end; the previous chunk becomes reusable
    int release_fd() { const int f = fd_; fd_ = -1; return f; }   // (before start(): the caller reads the input itself)
    const std::string &error() const { return error_; }
    double ms_read = 0;                                      // time in read(2), by the read-ahead thread
private:
    void producer();
    int fd_ = -1;
    std::vector<uint8_t> head_;
    size_t chunk_bytes_ = 0;
    Chunk ring_[3];
    int head_i_ = 0, tail_i_ = 0, count_ = 0; Chunk *lent_ = nullptr;
    bool eof_ = false; std::atomic<bool> stop_{false}; std::string error_;
    std::mutex mu_; std::condition_variable cv_;
    std::thread th_;
};

}  // namespace rsqc_host
