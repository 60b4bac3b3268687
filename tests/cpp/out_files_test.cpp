// out_files_test -- the temp-then-rename file set of secedo_amd/csrc/out_files.hpp on the host, under AddressSanitizer
// and UBSan, in a temporary directory and in both keep_open modes: append and commit, the removal of what was not
// committed (the files, a directory it made, not one that was there), a target under a directory that does not exist,
// a rename onto a non-empty directory, the order of the bytes of two appends, an empty append, and the refusals of
// open()'s directory. Prints "ok <n> checks" and exits 0, or names the first check that failed.
#include "out_files.hpp"

#include <dirent.h>
#include <ftw.h>

#include <cstdlib>
#include <fstream>
#include <iterator>

using secedo::host::OutFiles;

namespace {

int g_checks = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

bool exists(const std::string &path) {
    struct stat st;
    return stat(path.c_str(), &st) == 0;
}

// the bytes of a file; "<missing>" where there is none
std::string slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return "<missing>";
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// the entries of a directory whose names hold `part`; -1 where it cannot be read
int count_entries(const std::string &dir, const std::string &part) {
    DIR *d = opendir(dir.c_str());
    if (!d) return -1;
    int n = 0;
    while (const dirent *e = readdir(d)) {
        const std::string name = e->d_name;
        if (name != "." && name != ".." && name.find(part) != std::string::npos) ++n;
    }
    closedir(d);
    return n;
}

int run_mode(const std::string &root, bool keep_open) {
    const std::string base = root + (keep_open ? "/open" : "/reopen");
    CHECK(mkdir(base.c_str(), 0777) == 0);
    const std::string pid = ".tmp." + std::to_string(long(getpid()));

    // append and commit: two appends concatenate in order, an empty append is a no-op
    {
        OutFiles of;
        of.keep_open = keep_open;
        of.target = {base + "/a.txt", base + "/b.bin", base + "/empty"};
        CHECK(of.open().empty());
        CHECK(of.tmp.size() == 3 && of.tmp[0] == base + "/a.txt" + pid && of.tmp[2] == base + "/empty" + pid);
        CHECK(exists(of.tmp[0]) && exists(of.tmp[1]) && exists(of.tmp[2]) && !exists(of.target[0]));
        CHECK(of.append(0, "first ", 6).empty());
        CHECK(of.append(1, "\0\1\2", 3).empty());
        CHECK(of.append(0, nullptr, 0).empty());
        CHECK(of.append(0, "second", 6).empty());
        CHECK(of.append(2, "", 0).empty());
        CHECK(!exists(of.target[0]) && !exists(of.target[1]));  // nothing is renamed before commit()
        CHECK(of.commit().empty());
        CHECK(slurp(of.target[0]) == "first second");
        CHECK(slurp(of.target[1]) == std::string("\0\1\2", 3));
        CHECK(slurp(of.target[2]).empty());
    }
    CHECK(count_entries(base, ".tmp.") == 0 && count_entries(base, "") == 3);  // the destructor left the targets

    // commit() replaces a target that is there
    {
        OutFiles of;
        of.keep_open = keep_open;
        of.target = {base + "/a.txt"};
        CHECK(of.open().empty() && of.append(0, "new", 3).empty());
        CHECK(slurp(of.target[0]) == "first second");
        CHECK(of.commit().empty());
        CHECK(slurp(of.target[0]) == "new");
    }

    // destruct without commit: the temporary files go, a directory open() made goes, one that was there stays
    const std::string made = base + "/made", there = base + "/there";
    CHECK(mkdir(there.c_str(), 0777) == 0);
    for (const std::string &dir : {made, there}) {
        {
            OutFiles of;
            of.keep_open = keep_open;
            of.dir = dir;
            of.target = {dir + "/x", dir + "/y"};
            CHECK(of.open().empty());
            CHECK(of.append(1, "bytes", 5).empty());
            CHECK(count_entries(dir, ".tmp.") == 2);
        }
        CHECK(exists(dir) == (dir == there));
    }
    CHECK(count_entries(there, "") == 0);
    // a directory open() made stays once committed
    {
        OutFiles of;
        of.keep_open = keep_open;
        of.dir = made;
        of.target = {made + "/x"};
        CHECK(of.open().empty() && of.append(0, "x", 1).empty() && of.commit().empty());
    }
    CHECK(slurp(made + "/x") == "x" && count_entries(made, "") == 1);

    // open()'s directory: a file in its place, a parent that does not exist
    {
        OutFiles of;
        of.keep_open = keep_open;
        of.dir = base + "/a.txt";
        of.target = {of.dir + "/x"};
        CHECK(of.open() == base + "/a.txt is not a directory");
    }
    CHECK(slurp(base + "/a.txt") == "new");
    {
        OutFiles of;
        of.keep_open = keep_open;
        of.dir = base + "/none/depth";
        of.target = {of.dir + "/x"};
        CHECK(of.open() == "Could not create " + base + "/none/depth");
    }
    CHECK(!exists(base + "/none"));

    // a target under a directory that does not exist: open() says so and nothing is left, of the file before it neither
    {
        OutFiles of;
        of.keep_open = keep_open;
        of.target = {base + "/before", base + "/none/x"};
        CHECK(of.open() == "Could not write " + base + "/none/x" + pid);
    }
    CHECK(!exists(base + "/none") && !exists(base + "/before") && count_entries(base, ".tmp.") == 0);

    // a rename onto a non-empty directory fails: the words, the target before it is complete, the rest is removed
    const std::string full = base + "/full";
    CHECK(mkdir(full.c_str(), 0777) == 0);
    CHECK(std::ofstream(full + "/inside").put('i').good());
    {
        OutFiles of;
        of.keep_open = keep_open;
        of.target = {base + "/r0", full, base + "/r2"};
        CHECK(of.open().empty());
        CHECK(of.append(0, "zero", 4).empty() && of.append(1, "one", 3).empty() && of.append(2, "two", 3).empty());
        CHECK(of.commit() == "Could not rename " + full + pid + " to " + full);
    }
    CHECK(slurp(base + "/r0") == "zero" && !exists(base + "/r2") && count_entries(base, ".tmp.") == 0);
    CHECK(slurp(full + "/inside") == "i");
    return 0;
}

int run() {
    const char *tmp = std::getenv("TMPDIR");
    std::string root = std::string(tmp && *tmp ? tmp : "/tmp") + "/out_files_test.XXXXXX";
    CHECK(mkdtemp(&root[0]) != nullptr);
    const int rc = run_mode(root, true) || run_mode(root, false);
    const auto drop = [](const char *path, const struct stat *, int, struct FTW *) { return remove(path); };
    CHECK(nftw(root.c_str(), drop, 16, FTW_DEPTH | FTW_PHYS) == 0 || rc);
    return rc;
}

}  // namespace

int main() {
    if (run()) return 1;
    std::printf("ok %d checks\n", g_checks);
    return 0;
}
