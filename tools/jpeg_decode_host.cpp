// The JPEG decoder of csrc/jpeg_dec.hip on the host, for sanitizer runs: the same entropy decoder, ISLOW pass,
// upsampling and colour functions (csrc/jpeg_dec_core.hpp), driven by loops instead of launches.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/jpeg_decode_host.cpp -o jpeg_decode_host
//   jpeg_decode_host TABLES OUT.rgb FILE.jpg [FILE.jpg ...]
//
// TABLES is what s2v_amd.mjpeg.pack_streams builds for the files, up to its "data" part, behind a header of 16
// int32: magic 'S2VJ', n, h, w, sampling, intervals, max_per_frame, sets, then the byte offsets of intervals,
// frame_first, set_index, qtables and huff_sets in the rest of the file, the data byte count, and two zeros.
// The files' bytes, end to end, are the data.  OUT.rgb gets n frames of h x w RGB; "status B S" lines go to stdout.
// Every buffer is allocated at its exact size, so a read or write past one is a sanitizer report.
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
    fprintf(stderr, "jpeg_decode_host: %s\n", what);
    exit(2);
}

// a part of the tables file as its own exact-size allocation
template <class T>
static std::vector<T> part(const std::vector<unsigned char> &t, long off, long count) {
    const long begin = 64 + off;
    if (off < 0 || count < 0 || begin + count * (long)sizeof(T) > (long)t.size()) fail("tables file too short");
    std::vector<T> v((size_t)count);
    if (count) memcpy(v.data(), t.data() + begin, (size_t)count * sizeof(T));
    return v;
}

int main(int argc, char **argv) {
    if (argc < 4) fail("usage: jpeg_decode_host TABLES OUT.rgb FILE.jpg [FILE.jpg ...]");
    const std::vector<unsigned char> t = read_file(argv[1]);
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
    const std::vector<unsigned short> qt = part<unsigned short>(t, hd[11], (long)n * 3 * 64);
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
    // ---- entropy: what jpeg_entropy_decode_lane does, one interval after the other
    std::vector<HuffTable> tab(HUFF_SET_TABLES);
    for (int iv_i = 0; iv_i < n_intervals; ++iv_i) {
        const Interval iv = load_interval(a, iv_i);
        if (!iv.ok) {
            for (int b = 0; b < n; ++b) status[b] = status[b] > ST_BAD_TABLE ? status[b] : (int)ST_BAD_TABLE;
            continue;
        }
        const int set = set_index[iv.frame];
        int err = ST_BAD_TABLE;
        if (set >= 0 && set < n_sets) {
            const unsigned char *spec = sets.data() + (long)set * HUFF_SET_BYTES;
            for (int k = 0; k < HUFF_SET_TABLES; ++k) huff_derive_codes(spec + k * HUFF_SPEC_BYTES, tab[k]);
            for (int i = 0; i < HUFF_SET_TABLES * 256; ++i)
                huff_derive_entry(spec + (i >> 8) * HUFF_SPEC_BYTES, tab[i >> 8], i & 255);
            err = decode_interval(a, iv, tab.data());
        }
        if (err > status[iv.frame]) status[iv.frame] = err;
    }
    // ---- IDCT: what jpeg_idct does, into planes at their padded sizes
    std::vector<unsigned char> yp((size_t)n * d.ph * d.pw), cbp((size_t)n * d.cph * d.cpw), crp(cbp.size());
    int nat_of_zz[64];
    for (int s = 0, z = 0; s < 15; ++s)
        for (int k = 0; k <= s; ++k) {
            const int r = (s & 1) ? k : s - k, c = s - r;
            if (r < 8 && c < 8) nat_of_zz[z++] = r * 8 + c;
        }
    for (int b = 0; b < n; ++b)
        for (int mcu = 0; mcu < d.mcus; ++mcu) {
            const int my = mcu / d.mcols, mx = mcu - my * d.mcols;
            for (int k = 0; k < d.bpm; ++k) {
                const int comp = block_component(k, d.hs, d.vs);
                const short *src = coef.data() + (((long)b * d.mcus + mcu) * d.bpm + k) * 64;
                long long x[64], tcol[64], in[8], o[8];
                for (int z = 0; z < 64; ++z)
                    x[nat_of_zz[z]] = (long long)src[z] * qt[((long)b * 3 + comp) * 64 + z];
                for (int c = 0; c < 8; ++c) {
                    for (int r = 0; r < 8; ++r) in[r] = x[r * 8 + c];
                    idct_islow_pass(in, o);
                    for (int r = 0; r < 8; ++r) tcol[r * 8 + c] = (int)((o[r] + 1024) >> 11);
                }
                for (int r = 0; r < 8; ++r) {
                    idct_islow_pass(tcol + r * 8, o);
                    unsigned char *dst;
                    if (comp == 0) {
                        const int by = k / d.hs, bx = k - by * d.hs;
                        dst = yp.data() + ((long)b * d.ph + my * 8 * d.vs + by * 8 + r) * d.pw + mx * 8 * d.hs + bx * 8;
                    } else {
                        dst = (comp == 1 ? cbp : crp).data() + ((long)b * d.cph + my * 8 + r) * d.cpw + mx * 8;
                    }
                    for (int c = 0; c < 8; ++c) dst[c] = (unsigned char)clamp_u8(((o[c] + (1LL << 17)) >> 18) + 128);
                }
            }
        }
    // ---- upsampling and colour: what jpeg_upsample_color does
    std::vector<unsigned char> out((size_t)n * h * w * 3);
    for (int b = 0; b < n; ++b) {
        const long coff = (long)b * d.cph * d.cpw;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const int Y = yp[((long)b * d.ph + y) * d.pw + x];
                const int cb = chroma_sample(cbp.data() + coff, d.cpw, d.ch, d.cw, d.hs, d.vs, y, x) - 128;
                const int cr = chroma_sample(crp.data() + coff, d.cpw, d.ch, d.cw, d.hs, d.vs, y, x) - 128;
                int R, G, B;
                ycc_to_rgb(Y, cb, cr, R, G, B);
                unsigned char *q = out.data() + (((long)b * h + y) * w + x) * 3;
                q[0] = (unsigned char)R;
                q[1] = (unsigned char)G;
                q[2] = (unsigned char)B;
            }
    }
    FILE *f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) fail("cannot write the output");
    fclose(f);
    for (int b = 0; b < n; ++b) printf("status %d %d\n", b, status[b]);
    return 0;
}
