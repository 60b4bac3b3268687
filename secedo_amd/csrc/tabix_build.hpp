// tabix_build.hpp -- the tabix index writer (.tbi of a bgzip-compressed VCF), header-only, in plain host C++ that g++
// compiles alone (tests/cpp/tabix_build_test.cpp runs it under the sanitizers; tabix_api.cpp feeds it what the device's
// line pass, tabix_kernels.hip, found). A TBI is the per-reference body of a BAI behind another header, so the bins,
// chunks and windows are bam_index_build.hpp's Builder's; this file adds the names and the header.
//
// Per file the builder takes, in file order: the chromosome names in the order of their first data line (a name that
// comes back is refused: its lines would not be one block), the heads of the runs of consecutive data lines with one
// (name, bin), each with the virtual offset of its first line and that line's ordinal among the file's data lines,
// and the touched 16 kb windows. What is written (uncompressed, little endian; the caller compresses it as BGZF):
//   "TBI\1", n_ref, format 2 (VCF), col_seq 1, col_beg 2, col_end 0, meta '#', skip 0, l_nm, the names NUL-terminated,
//   per name the body bamindexbuild::Builder::append_ref writes (bins ascending, the pseudo-bin 37450 last with (start
//   of the first line, end of the last), (lines, 0); the linear index filled backward), n_no_coor = 0.
// Small bins are not merged into their parents as newer htslib does; both forms are valid tabix indexes.
// Whatever it is fed, the builder answers with bytes or with a reason, never with a read or write out of bounds.
#pragma once

#include "bam_index_build.hpp"

#include <unordered_set>

namespace secedo {
namespace tabixbuild {

constexpr uint32_t kFormatVcf = 2, kColSeq = 1, kColBeg = 2, kColEnd = 0, kMeta = '#', kSkip = 0;

struct Stats {
    uint64_t names = 0, bins = 0, chunks = 0, windows = 0, joined = 0;
};

class Builder {
public:
    Builder() : body_(0) { body_.allow_offset_zero(); }

    // The next name of the file, in first-appearance order. Empty on success.
    std::string add_name(const std::string &name) {
        if (name.find('\0') != std::string::npos) return "a chromosome name with a NUL byte";
        if (!seen_.insert(name).second) return "chromosome blocks not continuous";
        names_.push_back(name);
        body_.add_ref();
        return std::string();
    }
    uint32_t n_names() const { return uint32_t(names_.size()); }

    // A run head: the first data line of a run with one (name, bin); start: its virtual offset, ordinal: its number
    // among the file's data lines.
    std::string add_head(uint32_t name, uint32_t bin, uint64_t start, uint64_t ordinal) {
        if (name >= names_.size()) return "a head of an unknown name";
        return body_.add_head(bamindexbuild::Head{int32_t(name), bin, 0, start, ordinal});
    }

    std::string add_window(uint32_t name, uint32_t w, uint64_t start) {
        if (name >= names_.size()) return "a window of an unknown name";
        return body_.add_window(bamindexbuild::Window{int32_t(name), w, start});
    }

    // end: the virtual offset behind the last data line (the end of the data); n_lines: the file's data lines.
    std::string finish(uint64_t end, uint64_t n_lines, std::vector<uint8_t> *out, Stats *stats) {
        const std::string why = body_.close_runs(end, n_lines);
        if (!why.empty()) return why;
        out->clear();
        using B = bamindexbuild::Builder;
        B::put(out, "TBI\1", 4);
        uint32_t l_nm = 0;
        for (const std::string &n : names_) l_nm += uint32_t(n.size()) + 1;
        for (const uint32_t v : {uint32_t(names_.size()), kFormatVcf, kColSeq, kColBeg, kColEnd, kMeta, kSkip, l_nm})
            B::put32(out, v);
        for (const std::string &n : names_) B::put(out, n.c_str(), n.size() + 1);
        for (uint32_t r = 0; r < names_.size(); ++r) {
            const std::string bad = body_.append_ref(r, out);
            if (!bad.empty()) return bad;
        }
        B::put64(out, 0);  // n_no_coor: every data line of a VCF has a position
        const bamindexbuild::Stats &s = body_.stats();
        *stats = Stats{names_.size(), s.bins, s.chunks, s.windows, s.joined};
        return std::string();
    }

private:
    std::vector<std::string> names_;
    std::unordered_set<std::string> seen_;  // of names_: a file may hold very many names
    bamindexbuild::Builder body_;
};

}  // namespace tabixbuild
}  // namespace secedo
