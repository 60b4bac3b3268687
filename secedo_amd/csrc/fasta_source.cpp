// fasta_source.cpp -- the reference genome file opened, classified by content and, where a host function needs its
// text, inflated with zlib (see fasta_source.hpp).
#include "fasta_source.hpp"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <string_view>

namespace secedo {
namespace fasta_host {

namespace {
std::atomic<int> g_route{-1};
thread_local secedo_variant_fasta_info g_info;

// zlib raw inflate of member k into dst[isize]; empty on success, else the message's tail
std::string inflate_member(const Source &src, size_t k, uint8_t *dst) {
    return bm::inflate_member_zlib(src.file + src.members[k].payload(), src.members[k], dst);
}

// gzip members one after another through zlib's gzip wrapper, which checks each member's CRC32 and ISIZE
int inflate_gzip(const std::string &path, const uint8_t *p, size_t n, std::vector<uint8_t> *out) {
    z_stream z{};
    if (inflateInit2(&z, 15 + 16) != Z_OK) return fail(SECEDO_E_INVALID_ARG, path + ": inflateInit2 failed");
    out->clear();
    out->resize(std::max<size_t>(n * 4, 1 << 16));
    size_t at = 0, in = 0;
    int rc = Z_OK;
    bool ended = false;  // the input ends exactly behind a member
    while (in < n) {
        if (at == out->size()) out->resize(out->size() * 2);
        const size_t give = std::min<size_t>(n - in, 1u << 30), room = std::min<size_t>(out->size() - at, 1u << 30);
        z.next_in = const_cast<Bytef *>(p + in);
        z.avail_in = uInt(give);
        z.next_out = out->data() + at;
        z.avail_out = uInt(room);
        rc = inflate(&z, Z_NO_FLUSH);
        in += give - z.avail_in;
        at += room - z.avail_out;
        ended = false;
        if (rc == Z_STREAM_END) {
            ended = true;
            if (in < n && inflateReset(&z) != Z_OK) break;
        } else if (rc != Z_OK && !(rc == Z_BUF_ERROR && z.avail_out == 0)) {
            break;
        }
    }
    inflateEnd(&z);
    if (!ended || in != n)
        return fail(SECEDO_E_INVALID_ARG, path + ": gzip stream is truncated or corrupt (a member's data, CRC32 or ISIZE)");
    out->resize(at);
    return SECEDO_OK;
}

}  // namespace

Source::~Source() {
    if (file && file_bytes) munmap(const_cast<uint8_t *>(file), file_bytes);
}

secedo_variant_fasta_info &info() { return g_info; }

void set_route(int route) { g_route.store(route); }

int get_route() {
    int mode = g_route.load();
    if (mode >= 0) return mode;
    const char *e = std::getenv("SECEDO_FASTA");
    if (!e || !*e || std::strcmp(e, "host") == 0) return SECEDO_FASTA_HOST;
    if (std::strcmp(e, "device") == 0) return SECEDO_FASTA_DEVICE;
    return fail(SECEDO_E_INVALID_ARG, std::string("SECEDO_FASTA=") + e + ": expected host or device");
}

int fasta_route(bool *device) {
    const int mode = get_route();
    if (mode < 0) return mode;
    *device = mode == SECEDO_FASTA_DEVICE;
    return SECEDO_OK;
}

uint64_t batch_bytes() { return std::max<uint64_t>(env_u64("SECEDO_FASTA_BATCH_BYTES", 256ull << 20), 64); }

int open_source(const char *path, Source *src) {
    g_info = secedo_variant_fasta_info{};
    bool device = false;
    SECEDO_CALL(fasta_route(&device));  // an unknown SECEDO_FASTA fails every call that reads a FASTA
    if (!path || !std::filesystem::exists(path))
        return fail(SECEDO_E_INVALID_ARG, std::string("Reference genome ") + (path ? path : "(null)") + " does not exist");
    src->path = path;
    const int fd = ::open(path, O_RDONLY);
    struct stat st;
    if (fd < 0 || fstat(fd, &st) != 0) {
        if (fd >= 0) close(fd);
        return fail(SECEDO_E_INVALID_ARG, std::string("cannot read ") + path);
    }
    src->file_bytes = size_t(st.st_size);
    if (src->file_bytes) {
        void *m = mmap(nullptr, src->file_bytes, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) {
            close(fd);
            src->file_bytes = 0;
            return fail(SECEDO_E_INVALID_ARG, std::string("cannot read ") + path);
        }
        madvise(m, src->file_bytes, MADV_SEQUENTIAL);
        src->file = static_cast<const uint8_t *>(m);
    }
    close(fd);
    if (src->file_bytes < 2 || src->file[0] != 0x1f || src->file[1] != 0x8b) {
        src->kind = SECEDO_FASTA_KIND_TEXT;
        src->has_text = true;
        return SECEDO_OK;
    }
    uint32_t len = 0, isize = 0, xlen = 0;
    if (bm::member_header(src->file, src->file_bytes, 0, &len, &isize, &xlen) == bm::kNoMember) {
        src->kind = g_info.kind = SECEDO_FASTA_KIND_GZIP;
        SECEDO_CALL(inflate_gzip(src->path, src->file, src->file_bytes, &src->inflated));
        g_info.host_inflated_bytes = src->inflated.size();
        src->has_text = true;
        return SECEDO_OK;
    }
    src->kind = g_info.kind = SECEDO_FASTA_KIND_BGZF;
    const std::string why = bm::list_members(src->file, src->file_bytes, &src->members, &src->members_text);
    return why.empty() ? SECEDO_OK : fail(SECEDO_E_INVALID_ARG, src->path + ": " + why);
}

int inflate_bgzf_host(Source *src) {
    src->inflated.resize(src->members_text);
    uint64_t at = 0;
    for (size_t k = 0; k < src->members.size(); ++k) {
        const std::string err = inflate_member(*src, k, src->inflated.data() + at);
        if (!err.empty()) return bad_member(src->path, k, err);
        at += src->members[k].isize;
    }
    g_info.host_inflated_bytes += at;
    src->has_text = true;
    return SECEDO_OK;
}

bool first_word_has_maternal(const uint8_t *p, size_t n) {
    size_t b = 0;
    while (b < n && isspace(p[b])) ++b;
    size_t e = b;
    while (e < n && !isspace(p[e])) ++e;
    return std::string_view(reinterpret_cast<const char *>(p) + b, e - b).find("maternal") != std::string_view::npos;
}

int bgzf_is_diploid(const Source &src, bool *diploid) {
    std::vector<uint8_t> head;
    for (size_t k = 0; k < src.members.size(); ++k) {
        const size_t at = head.size();
        head.resize(at + src.members[k].isize);
        const std::string err = inflate_member(src, k, head.data() + at);
        if (!err.empty()) return bad_member(src.path, k, err);
        g_info.host_inflated_bytes += src.members[k].isize;
        size_t b = 0;
        while (b < head.size() && isspace(head[b])) ++b;
        while (b < head.size() && !isspace(head[b])) ++b;
        if (b < head.size()) break;  // the first word ends inside what is inflated
    }
    *diploid = first_word_has_maternal(head.data(), head.size());
    return SECEDO_OK;
}

}  // namespace fasta_host
}  // namespace secedo
