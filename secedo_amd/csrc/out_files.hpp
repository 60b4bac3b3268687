// out_files.hpp -- the files a call writes, once for every writer: each is written under a temporary name beside its
// target (<target>.tmp.<pid>) and renamed by commit(), which renames nothing before every file is complete. Whatever
// is left uncommitted is removed by the destructor, the directory too where open() made it. Host only, no HIP: the
// functions return "" or why they failed, and the caller puts its error code on it (text_out.hpp: out_error).
#pragma once

#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <string>
#include <vector>

namespace secedo {
namespace host __attribute__((visibility("hidden"))) {

struct OutFiles {
    std::vector<std::string> target, tmp;  // the caller fills target before open()
    std::string dir;        // "" or the directory of the targets, which open() makes where there is none
    bool keep_open = true;  // false: every append reopens its file ("ab"): there may be more files than descriptors
    OutFiles() = default;
    OutFiles(const OutFiles &) = delete;
    OutFiles &operator=(const OutFiles &) = delete;
    ~OutFiles() {
        for (FILE *x : f_)
            if (x) fclose(x);
        if (committed_) return;
        for (const std::string &t : tmp) (void)unlink(t.c_str());
        if (made_dir_) (void)rmdir(dir.c_str());
    }
    std::string open() {
        if (!dir.empty()) {
            struct stat st;
            if (stat(dir.c_str(), &st) != 0) {
                if (mkdir(dir.c_str(), 0777) != 0) return "Could not create " + dir;
                made_dir_ = true;
            } else if (!S_ISDIR(st.st_mode)) {
                return dir + " is not a directory";
            }
        }
        const std::string suffix = ".tmp." + std::to_string(long(getpid()));
        for (const std::string &t : target) {
            tmp.push_back(t + suffix);
            FILE *x = fopen(tmp.back().c_str(), "wb");
            if (!x) return "Could not write " + tmp.back();
            if (keep_open) f_.push_back(x);
            else if (fclose(x) != 0) return "Could not write " + tmp.back();
        }
        return std::string();
    }
    std::string append(size_t k, const void *p, size_t n) {
        if (n == 0) return std::string();
        FILE *x = keep_open ? f_[k] : fopen(tmp[k].c_str(), "ab");
        const bool ok = x && fwrite(p, 1, n, x) == n;
        if ((!keep_open && x && fclose(x) != 0) || !ok) return "Could not write " + tmp[k];
        return std::string();
    }
    std::string commit() {
        for (size_t k = 0; k < f_.size(); ++k) {
            const bool ok = fclose(f_[k]) == 0;
            f_[k] = nullptr;
            if (!ok) return "Could not write " + tmp[k];
        }
        // nothing is renamed before every file is complete; a rename that fails leaves the targets before it, which
        // are complete files, and the destructor removes the rest
        for (size_t k = 0; k < tmp.size(); ++k)
            if (rename(tmp[k].c_str(), target[k].c_str()) != 0)
                return "Could not rename " + tmp[k] + " to " + target[k];
        committed_ = true;
        return std::string();
    }

private:
    std::vector<FILE *> f_;  // with keep_open: the open files, null once closed
    bool made_dir_ = false, committed_ = false;
};

}  // namespace host
}  // namespace secedo
