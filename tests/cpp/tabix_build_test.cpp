// tabix_build_test -- secedo_amd/csrc/tabix_build.hpp on the host, under AddressSanitizer and UBSan.
//   tabix_build_test build <input> <index out>
//       <input> is text, one item per line, what the device's line pass hands the builder for one file:
//         M <coffset> <first inflated byte> <isize>     a BGZF member, in file order (optional)
//         T <inflated bytes> <file bytes>                after the members: offsets below are text offsets and go
//                                                        through voffset(); without it they are virtual
//         N <name>                                       the next chromosome name, in first-appearance order
//         H <name number> <bin> <start> <ordinal>        a run head, in file order
//         W <name number> <window> <start>
//         E <end> <n_data_lines>                         last: builds
//       writes the uncompressed index and prints "names n chunks c bins b joined j windows w bytes n", or prints
//       "rejected: <why>".
//   tabix_build_test cuts <input> <step>
//       the same on the prefixes of 0, step, 2 * step, ... bytes of the input and on all of it, each parsed from a
//       heap block of its exact size, so a read past the bytes is a sanitizer report. Prints "built a rejected b".
// Exit 0 unless the arguments are wrong or a file cannot be read or written.
#include "tabix_build.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

using secedo::bamindexbuild::Member;
using secedo::bamindexbuild::voffset;
using secedo::tabixbuild::Builder;
using secedo::tabixbuild::Stats;

namespace {

bool read_file(const char *path, std::vector<uint8_t> *out) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + got);
    const bool ok = !std::ferror(f);
    std::fclose(f);
    return ok;
}

// the space-separated fields of one line
std::vector<std::string> fields(const uint8_t *b, const uint8_t *e) {
    std::vector<std::string> out;
    while (b < e) {
        while (b < e && *b == ' ') ++b;
        const uint8_t *t = b;
        while (b < e && *b != ' ') ++b;
        if (b > t) out.emplace_back(reinterpret_cast<const char *>(t), size_t(b - t));
    }
    return out;
}

bool number(const std::string &s, uint64_t hi, uint64_t *v) {
    if (s.empty() || s.size() > 20) return false;
    for (const char c : s)
        if (c < '0' || c > '9') return false;
    if (s.size() == 20 && s > "18446744073709551615") return false;
    const unsigned long long x = std::strtoull(s.c_str(), nullptr, 10);
    if (x > hi) return false;
    *v = x;
    return true;
}

// Empty and *out = the index, or why not.
std::string build(const uint8_t *d, size_t n, std::vector<uint8_t> *out, Stats *stats) {
    Builder b;
    std::vector<Member> members;
    bool linear = false;
    uint64_t total = 0, file_bytes = 0;
    const auto at = [&](uint64_t v, uint64_t *res) {
        if (linear && v > total) return false;
        *res = linear ? voffset(members, total, file_bytes, v) : v;
        return true;
    };
    for (size_t o = 0; o < n;) {
        size_t e = o;
        while (e < n && d[e] != '\n') ++e;
        const std::vector<std::string> f = fields(d + o, d + e);
        const bool whole = e < n;  // a line without its '\n' is a cut one
        o = e + 1;
        if (f.empty()) continue;
        if (!whole) return "a cut line";
        uint64_t v[4] = {0, 0, 0, 0};
        if (f[0] == "M" && f.size() == 4 && !linear && number(f[1], UINT64_MAX >> 16, &v[0]) &&
            number(f[2], UINT64_MAX >> 1, &v[1]) && number(f[3], 65536, &v[2])) {
            if (!members.empty() && (v[0] <= members.back().coff || v[1] != members.back().out + members.back().isize))
                return "members out of order";
            members.push_back(Member{v[0], v[1], uint32_t(v[2])});
        } else if (f[0] == "T" && f.size() == 3 && !linear && number(f[1], UINT64_MAX >> 1, &v[0]) &&
                   number(f[2], UINT64_MAX >> 16, &v[1])) {
            if (!members.empty() && v[0] != members.back().out + members.back().isize) return "T differs from the members";
            total = v[0], file_bytes = v[1], linear = true;
        } else if (f[0] == "N" && f.size() == 2) {
            const std::string why = b.add_name(f[1]);
            if (!why.empty()) return why;
        } else if (f[0] == "H" && f.size() == 5 && number(f[1], UINT32_MAX, &v[0]) && number(f[2], UINT32_MAX, &v[1]) &&
                   number(f[3], UINT64_MAX, &v[2]) && number(f[4], UINT64_MAX, &v[3]) && at(v[2], &v[2])) {
            const std::string why = b.add_head(uint32_t(v[0]), uint32_t(v[1]), v[2], v[3]);
            if (!why.empty()) return why;
        } else if (f[0] == "W" && f.size() == 4 && number(f[1], UINT32_MAX, &v[0]) && number(f[2], UINT32_MAX, &v[1]) &&
                   number(f[3], UINT64_MAX, &v[2]) && at(v[2], &v[2])) {
            const std::string why = b.add_window(uint32_t(v[0]), uint32_t(v[1]), v[2]);
            if (!why.empty()) return why;
        } else if (f[0] == "E" && f.size() == 3 && number(f[1], UINT64_MAX, &v[0]) && number(f[2], UINT64_MAX, &v[1]) &&
                   at(v[0], &v[0])) {
            return b.finish(v[0], v[1], out, stats);
        } else {
            return "a bad line";
        }
    }
    return "no E line";
}

// build() on a copy of exactly n bytes
std::string run(const uint8_t *d, size_t n, std::vector<uint8_t> *out, Stats *stats) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
    if (n) std::memcpy(exact.get(), d, n);
    return build(exact.get(), n, out, stats);
}

}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    std::vector<uint8_t> in, out;
    Stats st;
    if (mode == "build" && argc == 4) {
        if (!read_file(argv[2], &in)) return 2;
        const std::string why = run(in.data(), in.size(), &out, &st);
        if (!why.empty()) {
            std::printf("rejected: %s\n", why.c_str());
            return 0;
        }
        FILE *f = std::fopen(argv[3], "wb");
        if (!f) return 2;
        const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
        if (std::fclose(f) != 0 || !ok) return 2;
        std::printf("names %llu chunks %llu bins %llu joined %llu windows %llu bytes %zu\n", (unsigned long long)st.names,
                    (unsigned long long)st.chunks, (unsigned long long)st.bins, (unsigned long long)st.joined,
                    (unsigned long long)st.windows, out.size());
        return 0;
    }
    if (mode == "cuts" && argc == 4) {
        if (!read_file(argv[2], &in)) return 2;
        const size_t step = std::max<size_t>(1, std::strtoul(argv[3], nullptr, 10));
        unsigned long built = 0, rejected = 0;
        for (size_t n = 0; n < in.size(); n += step) (run(in.data(), n, &out, &st).empty() ? built : rejected)++;
        (run(in.data(), in.size(), &out, &st).empty() ? built : rejected)++;
        std::printf("built %lu rejected %lu\n", built, rejected);
        return 0;
    }
    std::fprintf(stderr, "usage: tabix_build_test build <input> <index out> | cuts <input> <step>\n");
    return 2;
}
