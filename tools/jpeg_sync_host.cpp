// The sync entropy decoder of csrc/jpeg_dec.hip (jpeg_entropy_decode_sync) on the host, for sanitizer runs: the same
// step function F (csrc/jpeg_dec_core.hpp, sync_step), with the rounds, the scans and the write pass as loops, one
// "lane" after the other.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/jpeg_sync_host.cpp -o jpeg_sync_host
//   jpeg_sync_host TABLES SUB_BYTES FILE.jpg [FILE.jpg ...]
//
// TABLES is the file tools/jpeg_decode_host.cpp reads.  Output: "status B S" per frame, "rounds I R" per interval
// (the Jacobi rounds until one changed nothing) and "checksum X": FNV-1a (64 bit) over the int16 coefficients
// [n][mcus][blocks][64] as little-endian bytes.  Every buffer is allocated at its exact size, so a read or write past
// one is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../speech-to-video-mpp_amd/csrc/jpeg_dec_core.hpp"

using namespace s2v::jdec;

static std::vector<unsigned char> read_file(const char *path) {
    std::vector<unsigned char> v;
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    unsigned char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

static void fail(const char *what) {
    fprintf(stderr, "jpeg_sync_host: %s\n", what);
    exit(2);
}

template <class T>
static std::vector<T> part(const std::vector<unsigned char> &t, long off, long count) {
    const long begin = 64 + off;
    if (off < 0 || count < 0 || begin + count * (long)sizeof(T) > (long)t.size()) fail("tables file too short");
    std::vector<T> v((size_t)count);
    if (count) memcpy(v.data(), t.data() + begin, (size_t)count * sizeof(T));
    return v;
}

int main(int argc, char **argv) {
    if (argc < 4) fail("usage: jpeg_sync_host TABLES SUB_BYTES FILE.jpg [FILE.jpg ...]");
    const std::vector<unsigned char> t = read_file(argv[1]);
    const int sub = atoi(argv[2]);
    if (sub < SYNC_SUB_MIN || sub > SYNC_SUB_MAX || sub % 4) fail("SUB_BYTES: a multiple of 4 from 4 to 4096");
    if (t.size() < 64) fail("tables file too short");
    int hd[16];
    memcpy(hd, t.data(), 64);
    if (hd[0] != 0x4a563253) fail("bad magic");
    const int n = hd[1], h = hd[2], w = hd[3], sampling = hd[4], n_intervals = hd[5], n_sets = hd[7];
    Dims d;
    if (!dims(n, h, w, sampling, d) || n_intervals <= 0 || n_sets <= 0) fail("bad sizes");
    const std::vector<int> intervals = part<int>(t, hd[8], (long)n_intervals * INTERVAL_INTS);
    const std::vector<int> frame_first = part<int>(t, hd[9], n + 1);
    const std::vector<int> set_index = part<int>(t, hd[10], n);
    const std::vector<unsigned char> sets = part<unsigned char>(t, hd[12], (long)n_sets * HUFF_SET_BYTES);
    std::vector<unsigned char> data;
    for (int i = 3; i < argc; ++i) {
        const std::vector<unsigned char> f = read_file(argv[i]);
        data.insert(data.end(), f.begin(), f.end());
    }
    data.shrink_to_fit();
    if ((long)data.size() != hd[13] || argc - 3 != n) fail("the files are not the ones the tables were built for");

    std::vector<short> coef((size_t)n * d.mcus * d.bpm * 64, 0);
    std::vector<int> status((size_t)n, 0);
    EntropyArgs a{data.data(), (long)data.size(), intervals.data(), n_intervals, frame_first.data(), n, d.mcus,
                  d.hs, d.vs, d.bpm, sets.data(), n_sets, set_index.data(), coef.data(), status.data()};
    std::vector<HuffTable> tab(HUFF_SET_TABLES);
    for (int iv_i = 0; iv_i < n_intervals; ++iv_i) {
        const Interval iv = load_interval(a, iv_i);
        bool ok = iv.ok;
        if (ok && iv_i > 0) {
            const Interval before = load_interval(a, iv_i - 1);
            ok = before.ok && iv.off >= before.end;
        }
        if (!ok) {
            for (int b = 0; b < n; ++b) status[b] = status[b] > ST_BAD_TABLE ? status[b] : (int)ST_BAD_TABLE;
            continue;
        }
        const int set = set_index[iv.frame];
        if (set < 0 || set >= n_sets) {
            if (status[iv.frame] < ST_BAD_TABLE) status[iv.frame] = ST_BAD_TABLE;
            continue;
        }
        const unsigned char *spec = sets.data() + (long)set * HUFF_SET_BYTES;
        for (int k = 0; k < HUFF_SET_TABLES; ++k) huff_derive_codes(spec + k * HUFF_SPEC_BYTES, tab[k]);
        for (int i = 0; i < HUFF_SET_TABLES * 256; ++i)
            huff_derive_entry(spec + (i >> 8) * HUFF_SPEC_BYTES, tab[i >> 8], i & 255);
        // ---- resolve: the kernel's rounds, with its records at their exact size
        const long nsub = sync_subs(iv.end - iv.off, sub);
        std::vector<unsigned long long> cur((size_t)nsub + 1), nxt((size_t)nsub + 1), seen((size_t)nsub, ~0ULL);
        std::vector<SyncSummary> sums((size_t)nsub);
        for (long b = 0; b <= nsub; ++b) cur[b] = nxt[b] = sync_pack((iv.off + b * sub) * 8, 0, 0);
        long rounds = 0;
        for (long round = 0; round <= nsub; ++round) {
            bool changed = false;
            for (long b = 0; b < nsub; ++b) {
                const unsigned long long in = cur[b];
                unsigned long long out = cur[b + 1];
                if (in != seen[b]) {
                    const long lo = iv.off + b * sub, hi = lo + sub < iv.end ? lo + sub : iv.end;
                    out = sync_step(a.stream, iv.off, iv.end, lo, hi, in, tab.data(), a.hs, a.vs, a.bpm, sums[b], nullptr,
                                    0, 0, 0, 0, 0);
                    seen[b] = in;
                }
                nxt[b + 1] = out;
                changed = changed || out != cur[b + 1];
            }
            cur.swap(nxt);
            ++rounds;
            if (!changed) break;
        }
        printf("rounds %d %ld\n", iv_i, rounds);
        // ---- scan and write
        short *dst = coef.data() + ((long)iv.frame * a.mcus + iv.first) * a.bpm * 64;
        const long long total = (long long)iv.count * a.bpm;
        long long first = 0, err_at = -1;
        int err = ST_OK;
        unsigned p[3] = {0, 0, 0};
        for (long b = 0; b < nsub; ++b) {
            const SyncSummary &s = sums[b];
            if (s.err != ST_OK && first + s.err_block < total && (err_at < 0 || first + s.err_block < err_at)) {
                err_at = first + s.err_block;
                err = s.err;
            }
            if (first < total) {
                const long lo = iv.off + b * sub, hi = lo + sub < iv.end ? lo + sub : iv.end;
                SyncSummary unused;
                sync_step(a.stream, iv.off, iv.end, lo, hi, cur[b], tab.data(), a.hs, a.vs, a.bpm, unused, dst, first,
                          total, (int)p[0], (int)p[1], (int)p[2]);
            }
            first += s.blocks;
            for (int c = 0; c < 3; ++c) p[c] += (unsigned)s.dc[c];
        }
        if (err > status[iv.frame]) status[iv.frame] = err;
    }
    unsigned long long sum = 0xCBF29CE484222325ULL;
    for (size_t i = 0; i < coef.size(); ++i) {
        const unsigned v = (unsigned short)coef[i];
        sum = (sum ^ (v & 255u)) * 0x100000001B3ULL;
        sum = (sum ^ (v >> 8)) * 0x100000001B3ULL;
    }
    for (int b = 0; b < n; ++b) printf("status %d %d\n", b, status[b]);
    printf("checksum %016llx\n", sum);
    return 0;
}
