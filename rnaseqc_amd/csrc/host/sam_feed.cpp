#include "sam_feed.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "../../../include/rnaseqc_amd.h"

namespace rsqc_host {

const char *input_format_name(InputFormat f) {
    switch (f) {
    case InputFormat::Bam: return "BAM";
    case InputFormat::SamBgzf: return "BGZF-compressed SAM";
    case InputFormat::SamText: return "SAM text";
    case InputFormat::PlainGzip: return "gzip (not BGZF)";
    default: return "unknown";
    }
}

// SAM text: a header line, or a first line of at least 11 tab-separated fields whose QNAME starts with a character the spec
// allows ([!-?A-~]); an empty input or other bytes are no SAM
static bool looks_like_sam(const uint8_t *h, size_t n) {
    if (n == 0) return false;
    if (h[0] == '@') return true;
    if (h[0] < '!' || h[0] > '~') return false;
    size_t tabs = 0, i = 0;
    for (; i < n && h[i] != '\n' && tabs < 10; ++i) tabs += h[i] == '\t';
    return tabs >= 10 || i == n;                                        // (a first line longer than the bytes looked at: judged by the parse)
}

InputFormat sniff_format(const uint8_t *h, size_t n) {
    if (n < 2 || h[0] != 0x1f || h[1] != 0x8b) return looks_like_sam(h, n) ? InputFormat::SamText : InputFormat::Unknown;
    // BGZF: gzip with FEXTRA holding a BC subfield (SAM spec 4.1)
    bool bgzf = false;
    if (n >= 18 && h[2] == 8 && (h[3] & 4)) {
        const size_t xlen = (size_t)h[10] | ((size_t)h[11] << 8);
        for (size_t o = 0; o + 4 <= xlen && 12 + o + 4 <= n;) {
            const uint8_t *x = h + 12 + o;
            const size_t slen = (size_t)x[2] | ((size_t)x[3] << 8);
            if (x[0] == 'B' && x[1] == 'C' && slen == 2) bgzf = true;
            o += 4 + slen;
        }
    }
    if (!bgzf) return InputFormat::PlainGzip;
    // the first inflated bytes
    uint8_t out[4] = {0, 0, 0, 0};
    z_stream zs{};
    if (inflateInit2(&zs, 15 + 16) != Z_OK) return InputFormat::Unknown;
    zs.next_in = const_cast<uint8_t *>(h); zs.avail_in = (uInt)n;
    zs.next_out = out; zs.avail_out = sizeof out;
    int rc = Z_OK;
    while (zs.avail_out && rc == Z_OK) rc = inflate(&zs, Z_NO_FLUSH);
    const size_t got = sizeof out - zs.avail_out;
    inflateEnd(&zs);
    if (got == 4 && !memcmp(out, "BAM\1", 4)) return InputFormat::Bam;
    return got ? InputFormat::SamBgzf : InputFormat::Unknown;
}

InputFormat sniff_file(const std::string &path) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return InputFormat::Unopenable;
    std::vector<uint8_t> b(1 << 17);
    size_t got = 0;
    while (got < b.size()) { const ssize_t g = pread(fd, b.data() + got, b.size() - got, (off_t)got); if (g <= 0) break; got += (size_t)g; }
    close(fd);
    return sniff_format(b.data(), got);
}

void parse_sam_header(const char *t, size_t n, SamHeader &h, bool &complete) {
    complete = false;
    size_t a = 0;
    while (a < n) {
        if (t[a] != '@') { complete = true; return; }
        const char *nl = (const char *)memchr(t + a, '\n', n - a);
        if (!nl) return;
        size_t len = (size_t)(nl - (t + a));
        if (len && t[a + len - 1] == '\r') --len;
        ++h.lines;
        if (len >= 3 && !memcmp(t + a, "@SQ", 3) && (len == 3 || t[a + 3] == '\t')) {
            std::string sn; uint64_t ln = 0; bool have = false;
            for (size_t f = a + 3; f < a + len;) {
                size_t e = f + 1;
                while (e < a + len && t[e] != '\t') ++e;
                const std::string field(t + f + 1, e - f - 1);
                if (field.compare(0, 3, "SN:") == 0) { sn = field.substr(3); have = true; }
                else if (field.compare(0, 3, "LN:") == 0) ln = strtoull(field.c_str() + 3, nullptr, 10);
                f = e;
            }
            if (have) { h.names.push_back(sn); h.lengths.push_back(ln); }
        }
        a = (size_t)(nl - t) + 1;
    }
    complete = a >= n ? false : true;
}

bool read_sam_header(const std::string &path, SamHeader &h) {
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) return false;
    std::string text;
    std::vector<char> buf(1 << 16);
    bool complete = false;
    for (;;) {
        const int got = gzread(f, buf.data(), (unsigned)buf.size());
        if (got < 0) { gzclose(f); return false; }
        text.append(buf.data(), (size_t)got);
        SamHeader t;
        parse_sam_header(text.data(), text.size(), t, complete);
        if (complete || got == 0) { h = t; break; }
        if (text.size() > ((size_t)1 << 32)) { gzclose(f); return false; }
    }
    gzclose(f);
    return true;
}

// ---- plain SAM feeder ------------------------------------------------------------------------------------------------
SamTextFeeder::~SamTextFeeder() {
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
    cv_.notify_all();
    if (th_.joinable()) th_.join();
    for (auto &c : ring_) if (c.data) { if (c.pinned) rsqc_host_free(c.data); else free(c.data); }
    if (fd_ >= 0) close(fd_);
}

bool SamTextFeeder::open(const std::string &path) {
    // the next file on the same feeder (a cohort): the reader of the file before is stopped first; the chunk buffers stay
    { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
    cv_.notify_all();
    if (th_.joinable()) th_.join();
    if (fd_ >= 0) { close(fd_); fd_ = -1; }
    head_.clear();
    head_i_ = tail_i_ = count_ = 0; lent_ = nullptr; eof_ = false; stop_ = false; error_.clear(); ms_read = 0;
    fd_ = ::open(path.c_str(), O_RDONLY);
    return fd_ >= 0;
}

const std::vector<uint8_t> &SamTextFeeder::peek(size_t n) {
    while (head_.size() < n) {
        const size_t at = head_.size();
        head_.resize(n);
        const ssize_t g = read(fd_, head_.data() + at, n - at);
        head_.resize(at + (g > 0 ? (size_t)g : 0));
        if (g <= 0) break;
    }
    return head_;
}

void SamTextFeeder::start(size_t chunk_bytes) {
    chunk_bytes_ = std::max<size_t>(chunk_bytes, head_.size() + 1);
    for (auto &c : ring_) {
        c.cap = chunk_bytes_;
        if (c.data && c.alloc >= c.cap) continue;                           // (page-locked for a file before this one)
        if (c.data) { if (c.pinned) rsqc_host_free(c.data); else free(c.data); }
        c.data = (uint8_t *)rsqc_host_alloc(c.cap);
        c.pinned = c.data != nullptr;
        if (!c.data) c.data = (uint8_t *)malloc(c.cap);
        c.alloc = c.cap;
    }
    th_ = std::thread([this] { producer(); });
}

void SamTextFeeder::producer() {
    bool first = true;
    for (;;) {
        Chunk *c;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return stop_ || count_ < 3; });
            if (stop_) return;
            c = &ring_[tail_i_];
        }
        size_t got = 0;
        if (first) { memcpy(c->data, head_.data(), head_.size()); got = head_.size(); first = false; }
        const auto t0 = std::chrono::steady_clock::now();
        bool end = false;
        while (got < c->cap) {
            if (stop_) return;                                              // (the consumer has gone: a pipe need not be drained)
            const ssize_t g = read(fd_, c->data + got, std::min<size_t>(c->cap - got, (size_t)1 << 20));
            if (g < 0) { std::lock_guard<std::mutex> lk(mu_); error_ = std::string("read failed: ") + strerror(errno); end = true; break; }
            if (g == 0) { end = true; break; }
            got += (size_t)g;
        }
        ms_read += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        c->bytes = got;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (got) { tail_i_ = (tail_i_ + 1) % 3; ++count_; }
            if (end) eof_ = true;
        }
        cv_.notify_all();
        if (end) return;
    }
}

SamTextFeeder::Chunk *SamTextFeeder::next() {
    std::unique_lock<std::mutex> lk(mu_);
    if (lent_) { head_i_ = (head_i_ + 1) % 3; --count_; lent_ = nullptr; cv_.notify_all(); }
    cv_.wait(lk, [&] { return count_ > 0 || eof_; });
    if (!count_) return nullptr;
    lent_ = &ring_[head_i_];
    return lent_;
}

}  // namespace rsqc_host
