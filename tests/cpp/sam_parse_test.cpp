// sam_parse_test.cpp -- TEST INFRASTRUCTURE ONLY: the SAM parser of secedo_amd/csrc/sam_parse.hpp as a host program
// under ASan and UBSan (tests/test_sam_parse_cpu.py runs it on the cases of tests/sam_cases.py and compares every
// byte with tests/sam_ref.py). It does what the four kernels of sam_kernels.hip do on one range of text: newline
// count per 16-byte vector, exclusive scan, line starts, the counting pass over every line, the writing pass over the
// selected lines below the first bad one.
//
// Every line is copied into a heap block of exactly its length before it is parsed, and every record is written into
// a block of exactly its counted size, so a read past a line's end, or a writing pass that disagrees with the counting
// pass, is an ASan report.
//
// usage: sam_parse_test <cases> <results>
// cases:   u32 n_cases, then per case: u32 n_names, (u32 length, bytes) per name, u8 selected[n_names],
//          u64 line_base, u8 ends_file, u32 length, text
// results: per case: u32 n16, u32 count[n16], u32 n_lines, u32 start[n_lines + 1], (i32 ref, i32 pos, u64 size)
//          [n_lines], u64 error word, u32 lines written (those below the first bad one), u64 bytes, the records
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "sam_parse.hpp"

namespace sb = secedo::bam;

namespace {

struct Reader {
    std::vector<uint8_t> d;
    size_t o = 0;
    bool ok = true;
    const uint8_t *take(size_t n) {
        if (d.size() - o < n) {
            ok = false;
            return nullptr;
        }
        o += n;
        return d.data() + o - n;
    }
    template <class T>
    T get() {
        T v{};
        if (const uint8_t *p = take(sizeof(T))) std::memcpy(&v, p, sizeof(T));
        return v;
    }
};

struct Writer {
    std::vector<uint8_t> d;
    template <class T>
    void put(T v) {
        const uint8_t *p = reinterpret_cast<const uint8_t *>(&v);
        d.insert(d.end(), p, p + sizeof(T));
    }
};

// the @SQ names as upload_sam_refs of bam_input.cpp lays them out
struct Refs {
    std::vector<uint8_t> bytes, sel;
    std::vector<uint32_t> off{0}, id;
    std::vector<uint64_t> hash;
    void finish() {
        const uint32_t n = uint32_t(off.size() - 1);
        std::vector<std::pair<uint64_t, uint32_t>> hs(n);
        for (uint32_t r = 0; r < n; ++r) hs[r] = {sb::sam_name_hash(bytes.data() + off[r], off[r + 1] - off[r]), r};
        std::sort(hs.begin(), hs.end());
        for (const auto &h : hs) hash.push_back(h.first), id.push_back(h.second);
        if (sel.empty()) sel.push_back(0);
    }
    sb::SamRefs view() const {
        return sb::SamRefs{bytes.data(), off.data(), hash.data(), id.data(), sel.data(), uint32_t(off.size() - 1)};
    }
};

std::unique_ptr<uint8_t[]> exact_copy(const uint8_t *p, size_t n) {
    std::unique_ptr<uint8_t[]> b(new uint8_t[n]);
    if (n) std::memcpy(b.get(), p, n);
    return b;
}

bool run_case(Reader &in, Writer &out) {
    Refs refs;
    const uint32_t n_names = in.get<uint32_t>();
    for (uint32_t r = 0; r < n_names && in.ok; ++r) {
        const uint32_t len = in.get<uint32_t>();
        if (const uint8_t *p = in.take(len)) refs.bytes.insert(refs.bytes.end(), p, p + len);
        refs.off.push_back(uint32_t(refs.bytes.size()));
    }
    if (const uint8_t *p = in.take(n_names)) refs.sel.assign(p, p + n_names);
    const uint64_t line_base = in.get<uint64_t>();
    const bool ends_file = in.get<uint8_t>() != 0;
    const uint32_t len = in.get<uint32_t>();
    const uint8_t *text = in.take(len);
    if (!in.ok) return false;
    refs.finish();
    const sb::SamRefs R = refs.view();

    // the split: whole vectors of the zero-padded text, in a block that ends with the last vector
    const uint32_t n16 = (len + 15) / 16;
    std::unique_ptr<uint8_t[]> padded(new uint8_t[size_t(n16) * 16]());
    if (len) std::memcpy(padded.get(), text, len);
    auto words = [&](uint32_t i, uint32_t w[4]) { std::memcpy(w, padded.get() + size_t(i) * 16, 16); };
    std::vector<uint32_t> cnt(n16), scan(n16 + 1, 0);
    for (uint32_t i = 0; i < n16; ++i) {
        uint32_t w[4];
        words(i, w);
        cnt[i] = sb::vector_newlines(w);
        scan[i + 1] = scan[i] + cnt[i];
    }
    const bool trailing = len && text[len - 1] == '\n';
    const uint32_t n_lines = scan[n16] + (trailing ? 0 : 1);
    std::unique_ptr<uint32_t[]> start(new uint32_t[size_t(n_lines) + 1]);
    start[0] = 0;
    if (!trailing) start[n_lines] = len + 1;
    for (uint32_t i = 0; i < n16; ++i) {
        uint32_t w[4];
        words(i, w);
        sb::vector_starts(w, i, scan[i], start.get());
    }

    // the counting pass
    std::vector<sb::LineInfo> info(n_lines);
    unsigned long long err = ~0ull;
    for (uint32_t k = 0; k < n_lines; ++k) {
        const uint32_t b = start[k], n = start[k + 1] - 1 - b;
        sb::LineInfo li{sb::kSamNoRecord, 0, 0};
        uint32_t code = sb::kSamOk;
        if (!(n == 0 && ends_file && k + 1 == n_lines)) {
            const auto line = exact_copy(text + b, n);
            code = sb::parse_line<false>(line.get(), n, R, nullptr, &li);
        }
        if (code != sb::kSamOk) {
            err = std::min(err, (unsigned long long)(line_base + k) << 8 | code);
            li = sb::LineInfo{sb::kSamNoRecord, 0, 0};
        }
        if (!(li.ref >= 0 && R.sel[li.ref])) li.bytes = 0;
        info[k] = li;
    }

    // the writing pass over the lines below the first bad one
    const uint32_t limit = err == ~0ull ? n_lines : uint32_t((err >> 8) - line_base);
    std::vector<uint8_t> records;
    for (uint32_t k = 0; k < limit; ++k) {
        if (info[k].bytes == 0) continue;
        const uint32_t b = start[k], n = start[k + 1] - 1 - b;
        const auto line = exact_copy(text + b, n);
        std::unique_ptr<uint8_t[]> rec(new uint8_t[info[k].bytes]);
        sb::LineInfo li{};
        const uint32_t code = sb::parse_line<true>(line.get(), n, R, rec.get(), &li);
        if (code != sb::kSamOk || li.bytes != info[k].bytes || li.ref != info[k].ref || li.pos != info[k].pos) {
            std::fprintf(stderr, "line %u: the writing pass gives code %u, %llu bytes\n", k, code,
                         (unsigned long long)li.bytes);
            return false;
        }
        records.insert(records.end(), rec.get(), rec.get() + li.bytes);
    }

    out.put<uint32_t>(n16);
    for (uint32_t c : cnt) out.put<uint32_t>(c);
    out.put<uint32_t>(n_lines);
    for (uint32_t k = 0; k <= n_lines; ++k) out.put<uint32_t>(start[k]);
    for (const sb::LineInfo &li : info) out.put<int32_t>(li.ref), out.put<int32_t>(li.pos), out.put<uint64_t>(li.bytes);
    out.put<uint64_t>(err);
    out.put<uint32_t>(limit);
    out.put<uint64_t>(records.size());
    out.d.insert(out.d.end(), records.begin(), records.end());
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]);
        return 2;
    }
    Reader in;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) return std::perror(argv[1]), 2;
        uint8_t buf[1 << 16];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) in.d.insert(in.d.end(), buf, buf + n);
        std::fclose(f);
    }
    Writer out;
    const uint32_t n_cases = in.get<uint32_t>();
    for (uint32_t c = 0; c < n_cases; ++c)
        if (!run_case(in, out) || !in.ok) {
            std::fprintf(stderr, "case %u failed%s\n", c, in.ok ? "" : " (the case file is cut short)");
            return 1;
        }
    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return std::perror(argv[2]), 2;
    const bool written = std::fwrite(out.d.data(), 1, out.d.size(), f) == out.d.size();
    if (std::fclose(f) != 0 || !written) return std::perror(argv[2]), 2;
    std::printf("ok %u cases\n", n_cases);
    return 0;
}
