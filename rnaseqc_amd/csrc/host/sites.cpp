// sites.cpp -- see sites.hpp
#include "sites.hpp"

#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <numeric>
#include <unordered_map>

namespace rsqc_host {

namespace {

// POS: digits only (leading zeros are read over), 1 .. 2^31 - 1
bool parse_pos(const std::string &s, int32_t &pos0) {
    if (s.empty()) return false;
    uint64_t v = 0;
    for (char ch : s) {
        if (ch < '0' || ch > '9') return false;
        v = v * 10 + (uint64_t)(ch - '0');
        if (v > 2147483647ull) return false;                 // (before it can wrap)
    }
    if (v < 1) return false;
    pos0 = (int32_t)(v - 1);
    return true;
}

bool take_line(const std::string &path, uint64_t number, std::string &line, SiteFile &out, std::string &error) {
    while (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') return true;
    std::string f[5];
    size_t at = 0;
    for (int k = 0; k < 5; ++k) {
        if (at > line.size()) { error = path + ":" + std::to_string(number) + ": fewer than five tab-separated fields"; return false; }
        const size_t tab = line.find('\t', at);
        f[k] = line.substr(at, tab == std::string::npos ? std::string::npos : tab - at);
        at = tab == std::string::npos ? line.size() + 1 : tab + 1;
    }
    SiteLine s;
    if (!parse_pos(f[1], s.pos)) { error = path + ":" + std::to_string(number) + ": POS is not an integer in 1 .. 2147483647: " + f[1]; return false; }
    if (f[3].size() != 1 || !strchr("ACGTacgt", f[3][0])) { ++out.skipped_lines; return true; }
    s.chrom = std::move(f[0]); s.id = std::move(f[2]); s.ref = std::move(f[3]); s.alt = std::move(f[4]);
    out.lines.push_back(std::move(s));
    return true;
}

}  // namespace

int read_sites(const std::string &path, SiteFile &out, std::string &error) {
    out = SiteFile{};
    gzFile gz = gzopen(path.c_str(), "rb");                 // (plain files are read as they are)
    if (!gz) { error = path; return 10; }
    (void)gzbuffer(gz, 1u << 18);
    std::vector<char> buf(1u << 16);
    std::string line;
    uint64_t number = 1;
    int rc = 0;
    for (;;) {
        const int got = gzread(gz, buf.data(), (unsigned)buf.size());
        if (got < 0) { error = path + ": read error"; rc = 10; break; }
        if (got == 0) {
            if (!line.empty() && !take_line(path, number, line, out, error)) rc = 11;
            break;
        }
        int a = 0;
        for (int k = 0; k < got && !rc; ++k) {
            if (buf[(size_t)k] != '\n') continue;
            line.append(buf.data() + a, (size_t)(k - a));
            if (!take_line(path, number, line, out, error)) rc = 11;
            line.clear(); a = k + 1; ++number;
        }
        if (rc) break;
        line.append(buf.data() + a, (size_t)(got - a));
    }
    gzclose(gz);
    return rc;
}

void resolve_sites(const SiteFile &file, const std::vector<std::string> &contigs, ResolvedSites &out) {
    out = ResolvedSites{};
    std::unordered_map<std::string, int32_t> index;
    for (size_t k = 0; k < contigs.size(); ++k) index.emplace(contigs[k], (int32_t)k);       // (a repeated name keeps its first place)
    std::vector<int32_t> tid_of(file.lines.size(), -1);
    std::vector<uint32_t> order;
    for (size_t k = 0; k < file.lines.size(); ++k) {
        const auto it = index.find(file.lines[k].chrom);
        if (it == index.end()) { ++out.off_header_lines; continue; }
        tid_of[k] = it->second;
        order.push_back((uint32_t)k);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return tid_of[a] != tid_of[b] ? tid_of[a] < tid_of[b] : file.lines[a].pos < file.lines[b].pos;
    });
    out.first.assign(contigs.size() + 1, 0);
    for (uint32_t k : order) {
        const int32_t tid = tid_of[k], pos = file.lines[k].pos;
        if (!out.tid.empty() && out.tid.back() == tid && out.pos.back() == pos) { ++out.duplicate_lines; continue; }
        out.tid.push_back(tid); out.pos.push_back(pos); out.line.push_back(k);
        out.first[(size_t)tid + 1] += 1;
    }
    for (size_t t = 0; t < contigs.size(); ++t) out.first[t + 1] += out.first[t];
}

}  // namespace rsqc_host
