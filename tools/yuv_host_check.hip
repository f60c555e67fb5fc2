// yuv_host_check.hip — the planner and the kernel body of kernels_resize_nv12.hip run as HOST code under the sanitizers.
//
// resize_yuv_body is a __host__ __device__ function of (workgroup, thread) with the barrier passed in, so this program runs the very
// text the GPU runs: 256 host threads, one per work-item, a real barrier, and every buffer (frames, plan, LDS, output) a heap block
// of exactly the size the contract gives it, so that AddressSanitizer sees any access one byte outside.  No device is touched.
//
// Build (host code only; a CPU tool, never run on a GPU machine under a sanitizer):
//   hipcc -x hip --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/yuv_host_check.hip -o tools/yuv_host_check -Lvit-fpga_amd -lvithip -Wl,-rpath,$PWD/vit-fpga_amd -lpthread
// (libvithip.so gives resize_axis_table_over, the merged axis table of kernels_resize.hip; the planner and the body are this
// program's own, sanitized copies.)
// Use: yuv_host_check CASE OUT.  tools/yuv_host_check.py writes the case files, runs this program over them and compares OUT with the
// fp32 emulation of tests/yuv_ref.py.
//
// CASE (little endian): int32 layout (bit 0: 1 = vh_frame_yuv descriptors, 0 = vh_frame_nv12; bit 1: 16-bit samples; bit 2: packed
// 4:2:2, vh_frame_yuy2 descriptors, bit 0 then unread; bit 3: the frames start one sample (1 or 2 bytes) into their heap block, so
// that the base itself is what breaks the macropixel alignment), S, batch, chroma_site; float m[12]; uint64 nbytes; the
// descriptors; nbytes of frames.  OUT: [batch][S][S][3] bytes.  Bit 4: packed 4:4:4, vh_frame_bgra descriptors and
// resize_packed444_body, bits 0 and 2 then unread; bits 8-10 of the word are then the number of bytes (0..7) the frames start into
// their heap block, so that the base takes every residue the one-load-per-pixel rule asks about.
// With 16-bit samples UBSan's alignment check watches every uint16_t and uint32_t load: the planner's even-offset rule (and its
// multiple-of-4 rule for the pair load) has to be what makes them aligned.  The same holds for the packed layouts' 32-bit and 64-bit
// macropixel loads and for v210's 32-bit words, and for the 32-bit and 64-bit pixel loads of the packed 4:4:4 body; its 3-byte pixels
// end an exact-size block, so that a load wider than a byte at the last pixel is an AddressSanitizer report.
#include <pthread.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#define VH_HOST_CHECK 1   // the source below without its __global__ wrapper and launchers
#include "../vit-fpga_amd/csrc/kernels_resize_nv12.hip"

namespace {

template <class T>
bool rd(FILE* f, T* v, size_t n = 1) { return fread(v, sizeof(T), n, f) == n; }

int die(const char* what) {
    fprintf(stderr, "yuv_host_check: %s\n", what);
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return die("usage: yuv_host_check CASE OUT");
    FILE* f = fopen(argv[1], "rb");
    if (!f) return die("cannot open the case file");
    int32_t layout, S, batch, site;
    float m[12];
    uint64_t nbytes;
    if (!rd(f, &layout) || !rd(f, &S) || !rd(f, &batch) || !rd(f, &site) || !rd(f, m, 12) || !rd(f, &nbytes) || batch < 1 || batch > 4096)
        return die("short case file");
    const bool p444 = layout & 16, packed = !p444 && (layout & 4), planar = !packed && !p444 && (layout & 1), wide = layout & 2;
    const size_t shift = p444 ? (size_t)((layout >> 8) & 7) : layout & 8 ? (wide ? 2 : 1) : 0;
    std::vector<vh_frame_yuv> dy(planar ? batch : 0);
    std::vector<vh_frame_nv12> dn(planar || packed || p444 ? 0 : batch);
    std::vector<vh_frame_yuy2> dp(packed ? batch : 0);
    std::vector<vh_frame_bgra> d4(p444 ? batch : 0);
    if (p444 ? !rd(f, d4.data(), (size_t)batch) : packed ? !rd(f, dp.data(), (size_t)batch) : planar ? !rd(f, dy.data(), (size_t)batch) : !rd(f, dn.data(), (size_t)batch))
        return die("short descriptors");
    uint8_t* block = (uint8_t*)malloc(nbytes + shift);               // exact size: the byte behind the last plane is poisoned
    uint8_t* frames = block + shift;
    if (!block || !rd(f, frames, (size_t)nbytes)) return die("short frames");
    fclose(f);

    std::vector<uint32_t> words;
    int max_tiles = 0;
    const uintptr_t base = (uintptr_t)frames;
    const char* why = p444 ? vh::resize_plan_build_bgra(d4.data(), batch, S, (size_t)nbytes, (unsigned)(base & 7), wide ? 2 : 1, &words, &max_tiles)
                    : packed ? vh::resize_plan_build_yuy2(dp.data(), batch, S, (size_t)nbytes, (unsigned)(base & 7), site, wide ? 2 : 1, &words, &max_tiles)
                    : planar ? vh::resize_plan_build_yuv(dy.data(), batch, S, (size_t)nbytes, (base & 1) == 0, site, wide ? 2 : 1, &words, &max_tiles)
                    : vh::resize_plan_build_nv12(dn.data(), batch, S, (size_t)nbytes, (unsigned)(base & 3), site, wide ? 2 : 1, &words, &max_tiles);
    if (why) {
        printf("refused: %s\n", why);
        return 3;
    }
    uint32_t* plan = (uint32_t*)malloc(words.size() * 4);
    memcpy(plan, words.data(), words.size() * 4);
    const size_t nout = (size_t)batch * S * S * 3;
    uint8_t* out = (uint8_t*)malloc(nout);
    memset(out, 0xA5, nout);
    float* lds = (float*)aligned_alloc(16, sizeof(float) * vh::kResizeLdsFloats);
    vh::Nv12Matrix mat;
    memcpy(mat.m, m, sizeof mat.m);

    // 256 threads play the work-items of one workgroup after the other; a second wait closes each workgroup, so that the next one's
    // horizontal pass does not overwrite LDS a slow thread still reads
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, 256);
    const int blocks = batch * max_tiles;
    auto item = [&](int tid) {
        auto barrier = [&] { pthread_barrier_wait(&bar); };
        for (int b = 0; b < blocks; ++b) {
            if (p444 && wide) vh::resize_packed444_body<uint16_t>(frames, plan, out, S, max_tiles, mat, lds, b, tid, barrier);
            else if (p444) vh::resize_packed444_body<uint8_t>(frames, plan, out, S, max_tiles, mat, lds, b, tid, barrier);
            else if (packed && wide) vh::resize_yuv_body<true, uint16_t, true>(frames, plan, out, S, max_tiles, mat, lds, b, tid, barrier);
            else if (packed) vh::resize_yuv_body<true, uint8_t, true>(frames, plan, out, S, max_tiles, mat, lds, b, tid, barrier);
            else if (planar && wide) vh::resize_yuv_body<true, uint16_t>(frames, plan, out, S, max_tiles, mat, lds, b, tid, barrier);
            else if (planar) vh::resize_yuv_body<true, uint8_t>(frames, plan, out, S, max_tiles, mat, lds, b, tid, barrier);
            else if (wide) vh::resize_yuv_body<false, uint16_t>(frames, plan, out, S, max_tiles, mat, lds, b, tid, barrier);
            else vh::resize_yuv_body<false, uint8_t>(frames, plan, out, S, max_tiles, mat, lds, b, tid, barrier);
            pthread_barrier_wait(&bar);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < 256; ++t) pool.emplace_back(item, t);
    for (std::thread& t : pool) t.join();
    pthread_barrier_destroy(&bar);

    int bands = 0, tiles = 0, wide_loads = 0;
    for (int b = 0; b < batch; ++b) {
        vh::RzNv12 r;
        memcpy(&r, plan + (size_t)b * vh::kResizeNv12FrameWords, sizeof r);
        const int nb = (S + r.band_rows - 1) / r.band_rows, nc = (S + r.tile_cols - 1) / r.tile_cols;
        if (nb > bands) bands = nb;
        if (nc > tiles) tiles = nc;
        wide_loads += r.uv16;
    }
    printf("ok: %d frame(s) -> %d, %zu plan words, %d workgroups (at most %d bands x %d column tiles a frame)", batch, S, words.size(), blocks, bands, tiles);
    if (packed) printf(", %d frame(s) with one load per macropixel", wide_loads);
    if (p444) printf(", %d frame(s) with one load per pixel, base %% 8 = %u", wide_loads, (unsigned)(base & 7));
    printf("\n");
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(out, 1, nout, g) != nout) return die("cannot write the output");
    fclose(g);
    free(lds); free(out); free(plan); free(block);
    return 0;
}
