// Sanitizer pass over the scan preparation of the device's entropy decoder (csrc/jpeg_host.h: prepare_scan, the only new host code
// that reads untrusted bytes; it walks markers and byte stuffing and decodes nothing).  Stand-alone: its own main, no GPU, no Python.
//
//   python scripts/jpeg_corpus.py /tmp/jpeg_corpus
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpeg_scan_check.cpp -o /tmp/jpeg_scan_check
//   /tmp/jpeg_scan_check /tmp/jpeg_corpus
//
// Every file of the corpus goes through parse_headers + prepare_scan; then, deterministically from a fixed seed, every truncation
// length and MUTATIONS single-byte mutations of the three smallest supported files with at least 600 bytes and of the smallest one
// with a restart interval.  The input lives in a heap block of exactly its size and the record in one of exactly scan_bound() bytes
// (and, a second time, in one a few bytes short of what the call needs: SM_ENOSPACE, nothing written past it), so a read or write
// one byte past either end is a report.  Checked on every input besides the sanitizers' silence:
//   * the call ends in prepared, unsupported or - short buffer only - no-space;
//   * what the prepare step refuses, the host decoder (decode_scan) refuses too: the marker checks are the decoder's own, no stricter;
//   * a prepared record is consistent: offsets inside rec_bytes <= scan_bound(), segments end to end inside the unstuffed bytes,
//     MCU ranges as the restart interval implies, at least 8 zero bytes behind the scan.
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
static long failures = 0;

static void fail(const char* what) {
    if (failures++ < 10) printf("FAIL: %s\n", what);
}

// 0 prepared, 1 unsupported
static int run(const uint8_t* bytes, size_t len) {
    uint8_t* in = (uint8_t*)malloc(len ? len : 1);  // exactly len bytes: the sanitizer sees any over-read
    if (len) memcpy(in, bytes, len);
    smjpeg::Frame* f = new smjpeg::Frame;
    int rc = 1;
    if (smjpeg::parse_headers(in, len, *f)) {
        const size_t cap = smjpeg::scan_bound(f->info, len);
        uint8_t* rec = (uint8_t*)aligned_alloc(16, cap);
        sm_jpeg_scan sc;
        rc = smjpeg::prepare_scan(in, len, *f, rec, cap, sc);
        if (rc != SM_OK && rc != SM_JPEG_UNSUPPORTED) fail("scan_bound() bytes did not suffice");
        if (rc == SM_OK) {
            if (sc.rec_bytes < 0 || (size_t)sc.rec_bytes > cap || sc.rec_bytes % 16) fail("rec_bytes");
            if (sc.scan_off < 0 || sc.scan_len < 0 || sc.scan_off + sc.scan_len + 8 > sc.rec_bytes) fail("scan range");
            if (sc.seg_off < 0 || sc.n_seg < 1 || (int64_t)sc.seg_off + (int64_t)sc.n_seg * 16 > sc.huff_off) fail("segment table range");
            if (sc.n_huff < 1 || sc.n_huff > 6 || sc.huff_off + sc.n_huff * SM_JPEG_HUFF_BYTES > sc.qt_off || sc.qt_off + 384 != sc.scan_off) fail("table range");
            for (int i = 0; i < 8; ++i)
                if (rec[sc.scan_off + sc.scan_len + i]) fail("padding behind the scan");
            const int64_t n_mcu = (int64_t)sc.mcus_x * sc.mcus_y, ri = sc.restart_interval > 0 ? sc.restart_interval : n_mcu;
            int64_t at = 0, mcu = 0;
            for (int k = 0; k < sc.n_seg; ++k) {
                sm_jpeg_segment s;
                memcpy(&s, rec + sc.seg_off + (size_t)k * sizeof(s), sizeof(s));
                if (s.byte_off != at || s.byte_len < 0 || s.mcu0 != mcu || s.mcus != std::min(ri, n_mcu - mcu)) fail("segment entry");
                at += s.byte_len, mcu += s.mcus;
            }
            if (at != sc.scan_len || mcu != n_mcu) fail("segments do not cover the scan");
            // a buffer a little short of what this file needs
            const size_t need = (size_t)sc.scan_off + smjpeg::align16(len - f->scan_pos + 8);
            if (need >= 16) {
                uint8_t* small = (uint8_t*)aligned_alloc(16, need - 16 ? need - 16 : 16);
                sm_jpeg_scan sc2;
                if (smjpeg::prepare_scan(in, len, *f, small, need - 16, sc2) != SM_ENOSPACE) fail("a short buffer was not refused");
                free(small);
            }
        } else if (f->info.coef_bytes <= ((int64_t)1 << 26)) {  // refused here: the host decoder must refuse as well
            int16_t* coef = (int16_t*)malloc((size_t)f->info.coef_bytes ? (size_t)f->info.coef_bytes : 1);
            if (smjpeg::decode_scan(in, len, *f, coef)) fail("the prepare step refused a file the host decoder takes");
            free(coef);
        }
        free(rec);
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
    printf("corpus: %zu files, %ld prepared, %ld unsupported\n", files.size(), counts[0], counts[1]);
    std::vector<size_t> pick, rst;
    for (size_t i = 0; i < files.size(); ++i) {
        if (run(files[i].data(), files[i].size()) != 0) continue;
        smjpeg::Frame* f = new smjpeg::Frame;
        smjpeg::parse_headers(files[i].data(), files[i].size(), *f);
        (f->restart_interval ? rst : pick).push_back(i);
        delete f;
    }
    auto by_size = [&](size_t a, size_t b) { return files[a].size() < files[b].size(); };
    pick.erase(std::remove_if(pick.begin(), pick.end(), [&](size_t i) { return files[i].size() < 600; }), pick.end());
    std::stable_sort(pick.begin(), pick.end(), by_size);
    std::stable_sort(rst.begin(), rst.end(), by_size);
    if (pick.size() > 3) pick.resize(3);
    if (!rst.empty()) pick.push_back(rst[0]);
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
        printf("%s (%zu bytes): truncations %ld prepared / %ld unsupported; mutations %ld prepared / %ld unsupported\n",
               std::filesystem::path(names[i]).filename().c_str(), d.size(), t[0], t[1], m[0], m[1]);
        if (t[0] != 0) fail("a truncated file was prepared: it lacks its EOI at least");
    }
    if (failures) {
        printf("%ld failures\n", failures);
        return 1;
    }
    printf("ok: every input ended in prepared or unsupported, every record was consistent, no sanitizer report\n");
    return 0;
}
