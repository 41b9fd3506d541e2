// Stand-alone driver of csrc/dgp_jpeg_host.h for sanitizer builds (tests/test_jpeg_cpu.py compiles it with
// -fsanitize=address,undefined): parses and entropy-decodes every file of the directory given on the command line into buffers sized
// EXACTLY from the stream's own geometry, and ignores decode errors.  Exit status 0 = the decoder returned for every file without the
// sanitizers finding an out-of-range access or undefined arithmetic; 2 = usage / unreadable directory.
#include "../deepgraphpose_amd/csrc/dgp_jpeg_host.h"

#include <dirent.h>

#include <cstdio>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s DIRECTORY\n", argv[0]);
        return 2;
    }
    DIR* const dir = opendir(argv[1]);
    if (!dir) return 2;
    int files = 0, decoded = 0;
    while (const dirent* ent = readdir(dir)) {
        const std::string path = std::string(argv[1]) + "/" + ent->d_name;
        FILE* const f = std::fopen(path.c_str(), "rb");
        if (!f) continue;
        std::vector<uint8_t> raw;
        uint8_t chunk[4096];
        for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) raw.insert(raw.end(), chunk, chunk + got);
        std::fclose(f);
        if (raw.empty()) continue;
        ++files;
        // an exactly-sized heap copy: a read one byte past the stream is a heap-buffer-overflow
        std::vector<uint8_t> data(raw.begin(), raw.end());
        dgp_jpeg::State s;
        const char* why = "";
        if (!dgp_jpeg::parse(data.data(), (int64_t)data.size(), &s, &why)) continue;
        if (s.info.total_blocks > (1 << 16)) continue;      // (a corrupted size field: gigabytes of coefficients for a stream of a few KB)
        std::vector<int16_t> coef((size_t)s.info.total_blocks * 64);
        std::vector<uint16_t> qt((size_t)s.info.ncomp * 64);
        if (dgp_jpeg::entropy_decode(data.data(), (int64_t)data.size(), &s.info, coef.data(), qt.data(), &why)) ++decoded;
    }
    closedir(dir);
    std::printf("%d files, %d decoded\n", files, decoded);
    return 0;
}
