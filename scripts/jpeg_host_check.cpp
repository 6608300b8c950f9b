// Sanitizer pass over the host half of the JPEG decode (csrc/jpeg_host.h: the only code of the library that parses untrusted
// bytes).  Stand-alone: its own main, no GPU, no Python.
//
//   python scripts/jpeg_corpus.py /tmp/jpeg_corpus
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_host_check.cpp -o /tmp/jpeg_host_check
//   /tmp/jpeg_host_check /tmp/jpeg_corpus
//
// Every file of the corpus goes through the parser and the entropy decoder; then, deterministically from a fixed seed, every
// truncation length and MUTATIONS single-byte mutations of the three smallest supported files with at least 600 bytes.  Inputs and
// outputs live in heap blocks of exactly their size, so a read or write one byte past either end is a report.  Every call must end
// in "decoded" or "unsupported"; the program exits 0 only then (and only without a sanitizer report, which aborts it).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../salient-object-detection_amd/csrc/jpeg_host.h"

static const int MUTATIONS = 4000;

// 0 decoded, 1 unsupported; what sm_jpeg_entropy_decode does around the same two calls
static int run(const uint8_t* bytes, size_t len) {
    uint8_t* in = (uint8_t*)malloc(len ? len : 1);  // exactly len bytes: the sanitizer sees any over-read
    if (len) memcpy(in, bytes, len);
    smjpeg::Frame* f = new smjpeg::Frame;
    int rc = 1;
    if (smjpeg::parse_headers(in, len, *f)) {
        const size_t cb = (size_t)f->info.coef_bytes;
        if (cb <= ((size_t)1 << 28)) {  // a mutated size field may ask for gigabytes; the library's caller sizes its buffer from the probe too
            int16_t* coef = (int16_t*)malloc(cb ? cb : 1);
            uint16_t* qt = (uint16_t*)malloc(sizeof(uint16_t) * 64 * 3);
            if (smjpeg::decode_scan(in, len, *f, coef)) {
                smjpeg::write_tables(*f, qt);
                rc = 0;
            }
            free(qt);
            free(coef);
        }
    }
    delete f;
    free(in);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s CORPUS_DIR\n", argv[0]);
        return 2;
    }
    std::vector<std::string> names;
    for (auto& e : std::filesystem::directory_iterator(argv[1]))
        if (e.is_regular_file()) names.push_back(e.path().string());
    std::sort(names.begin(), names.end());
    std::vector<std::vector<uint8_t>> files;
    long counts[2] = {0, 0};
    for (auto& n : names) {
        std::ifstream s(n, std::ios::binary);
        std::vector<uint8_t> d((std::istreambuf_iterator<char>(s)), std::istreambuf_iterator<char>());
        counts[run(d.data(), d.size())]++;
        files.push_back(std::move(d));
    }
    printf("corpus: %zu files, %ld decoded, %ld unsupported\n", files.size(), counts[0], counts[1]);
    std::vector<size_t> pick;
    for (size_t i = 0; i < files.size(); ++i)
        if (files[i].size() >= 600 && run(files[i].data(), files[i].size()) == 0) pick.push_back(i);
    std::stable_sort(pick.begin(), pick.end(), [&](size_t a, size_t b) { return files[a].size() < files[b].size(); });
    if (pick.size() > 3) pick.resize(3);
    uint64_t rng = 0x9E3779B97F4A7C15ull;  // xorshift64, fixed seed
    auto next = [&]() {
        rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
        return rng;
    };
    for (size_t i : pick) {
        const std::vector<uint8_t>& d = files[i];
        long t[2] = {0, 0}, m[2] = {0, 0};
        for (size_t n = 0; n < d.size(); ++n) t[run(d.data(), n)]++;
        std::vector<uint8_t> w(d);
        for (int k = 0; k < MUTATIONS; ++k) {
            const size_t at = next() % d.size();
            const uint8_t v = (uint8_t)(next() & 255);
            w[at] = v;
            m[run(w.data(), w.size())]++;
            w[at] = d[at];
        }
        printf("%s (%zu bytes): truncations %ld decoded / %ld unsupported; mutations %ld decoded / %ld unsupported\n",
               std::filesystem::path(names[i]).filename().c_str(), d.size(), t[0], t[1], m[0], m[1]);
        if (t[0] != 0) {
            printf("FAIL: a truncated file decoded\n");
            return 1;
        }
    }
    printf("ok: every input ended in decoded or unsupported, no sanitizer report\n");
    return 0;
}
