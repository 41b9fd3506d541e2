// Stand-alone driver of the ENCODER half of csrc/dgp_jpeg_host.h for sanitizer builds (tests/test_jpeg_enc_cpu.py compiles it with
// -fsanitize=address,undefined).  Every file of the directory given on the command line is: int32 H, W, sampling, quality, then the
// frame's int16 coefficients.  Each is Huffman-coded from an exactly-sized heap copy into a heap buffer of exactly
// dgp_jpeg_encode_bound bytes, then into one of exactly the stream's length (must succeed) and one a byte shorter (must be refused), and
// the stream is decoded back (must give the coefficients).  Files with coefficients no category can code, a wrong length or a bad
// geometry must be refused.  Exit status 0 = all of that held and the sanitizers found nothing; 1 = a check failed; 2 = usage.
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
    int files = 0, encoded = 0, wrong = 0;
    while (const dirent* ent = readdir(dir)) {
        const std::string path = std::string(argv[1]) + "/" + ent->d_name;
        FILE* const f = std::fopen(path.c_str(), "rb");
        if (!f) continue;
        std::vector<uint8_t> raw;
        uint8_t chunk[4096];
        for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) raw.insert(raw.end(), chunk, chunk + got);
        std::fclose(f);
        if (raw.size() < 16) continue;
        ++files;
        int32_t head[4];
        memcpy(head, raw.data(), 16);
        const int32_t H = head[0], W = head[1], sampling = head[2], quality = head[3];
        uint16_t qt[128];
        const char* why = "";
        dgp_jpeg_info g;
        const bool geometry_ok = sampling != DGP_JPEG_GRAY && dgp_jpeg::geometry(W, H, sampling, &g);
        const int64_t bound = dgp_jpeg::encode_bound(H, W, sampling);
        if (!geometry_ok || !dgp_jpeg::quality_tables(quality, qt) || raw.size() != 16 + (size_t)g.total_blocks * 128) {
            // nothing to encode: the entry points must say so on their own
            std::vector<int16_t> none(64);
            std::vector<uint8_t> out(64);
            int64_t n = -1;
            if (!geometry_ok && (bound != 0 || dgp_jpeg::entropy_encode(none.data(), H, W, sampling, qt, out.data(), 64, &n, &why))) ++wrong;
            continue;
        }
        std::vector<int16_t> coef((size_t)g.total_blocks * 64);         // exactly sized: a read past the last block is a heap-buffer-overflow
        memcpy(coef.data(), raw.data() + 16, coef.size() * 2);
        std::vector<uint8_t> out((size_t)bound);
        int64_t n = -1;
        if (!dgp_jpeg::entropy_encode(coef.data(), H, W, sampling, qt, out.data(), bound, &n, &why)) {
            if (n != 0) ++wrong;
            continue;                                                    // (a coefficient outside its category: refused)
        }
        if (n <= 0 || n > bound) {
            ++wrong;
            continue;
        }
        ++encoded;
        std::vector<uint8_t> exact((size_t)n), shorter((size_t)n - 1);
        int64_t m = -1;
        if (!dgp_jpeg::entropy_encode(coef.data(), H, W, sampling, qt, exact.data(), n, &m, &why) || m != n ||
            memcmp(exact.data(), out.data(), (size_t)n) != 0)
            ++wrong;
        if (dgp_jpeg::entropy_encode(coef.data(), H, W, sampling, qt, shorter.data(), n - 1, &m, &why) || m != 0) ++wrong;
        dgp_jpeg::State s;
        std::vector<int16_t> back(coef.size());
        uint16_t qback[3 * 64];
        if (!dgp_jpeg::parse(exact.data(), n, &s, &why) || s.info.total_blocks != g.total_blocks ||
            !dgp_jpeg::entropy_decode(exact.data(), n, &s.info, back.data(), qback, &why)) {
            // (the decoder refuses streams in which some |coefficient x table entry| exceeds 32767: not an encoder fault)
            if (std::string(why).find("32767") == std::string::npos) ++wrong;
        } else if (memcmp(back.data(), coef.data(), coef.size() * 2) != 0 || memcmp(qback, qt, 128) != 0 || memcmp(qback + 64, qt + 64, 128) != 0) {
            ++wrong;
        }
    }
    closedir(dir);
    std::printf("%d files, %d encoded, %d wrong\n", files, encoded, wrong);
    return wrong ? 1 : 0;
}
