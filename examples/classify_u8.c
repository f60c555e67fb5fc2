/* classify_u8.c — 8-bit frames through the C ABI from plain C: the ring with u8 slots, normalisation on the GPU.
 *
 *   gcc -std=c99 -O2 -I include examples/classify_u8.c -L vit-fpga_amd -lvithip -Wl,-rpath,$PWD/vit-fpga_amd -o classify_u8
 *   ./classify_u8 [weights.vhblob | -] [batch] [frames]
 *
 * Pixel p of channel c enters the model as fmaf((float)p, scale[c], shift[c]) (one rounding; here the ImageNet mean / std),
 * so the logits are those vh_forward returns for that fp32 array.  A producer (decoder, camera) writes each batch of
 * `batch x H x W x C` bytes straight into the pinned buffer of the next slot; here a counter pattern stands in for it.
 * Without a file the weights are the seeded synthetic ones (seed 0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vithip.h"

#define CHECK(call, ctx)                                                        \
    do {                                                                        \
        if ((call) != VH_OK) {                                                  \
            fprintf(stderr, "%s: %s\n", #call, vh_last_error(ctx));             \
            return 1;                                                           \
        }                                                                       \
    } while (0)

static void report(const float* logits, int n, int classes, int frame) {
    for (int b = 0; b < n; ++b) {
        int best = 0;
        for (int c = 1; c < classes; ++c)
            if (logits[(size_t)b * classes + c] > logits[(size_t)b * classes + best]) best = c;
        printf("batch %d image %d: class %d (logit %.4f)\n", frame, b, best, logits[(size_t)b * classes + best]);
    }
}

int main(int argc, char** argv) {
    const char* path = (argc > 1 && strcmp(argv[1], "-") != 0) ? argv[1] : NULL;
    const int batch = argc > 2 ? atoi(argv[2]) : 8;
    const int frames = argc > 3 ? atoi(argv[3]) : 6;
    const int slots = 3;
    vh_config cfg = {224, 16, 3, 768, 12, 3072, 12, 1000, VH_DTYPE_BF16, 0, 1e-6f, 0};
    if (path) CHECK(vh_blob_file_config(path, &cfg), NULL);   /* model shape from the file's header */
    cfg.max_batch = batch;
    if (cfg.channels != 3) { fprintf(stderr, "this example normalises 3-channel images\n"); return 1; }
    vh_ctx* ctx = NULL;
    CHECK(vh_create(&cfg, 0, &ctx), NULL);
    if (path) CHECK(vh_load_weights_file(ctx, path), ctx);
    else CHECK(vh_init_weights_seeded(ctx, 0), ctx);

    /* (p / 255 - mean) / std  =  p * 1 / (255 std) + (-mean / std) */
    const double mean[3] = {0.485, 0.456, 0.406}, std[3] = {0.229, 0.224, 0.225};
    float scale[3], shift[3];
    for (int c = 0; c < 3; ++c) { scale[c] = (float)(1.0 / (255.0 * std[c])); shift[c] = (float)(-mean[c] / std[c]); }
    CHECK(vh_set_input_norm(ctx, scale, shift), ctx);

    const size_t in_bytes = (size_t)batch * cfg.image_size * cfg.image_size * cfg.channels;
    float* logits = (float*)malloc((size_t)batch * cfg.classes * sizeof(float));
    CHECK(vh_ring_create_u8(ctx, slots, batch), ctx);
    int submitted = 0, collected = 0, n = 0, free_slots = 0;
    while (collected < frames) {
        CHECK(vh_ring_free_slots(ctx, &free_slots), ctx);
        if (submitted < frames && free_slots > 0) {
            uint8_t* slot = NULL;
            CHECK(vh_ring_input_u8(ctx, &slot), ctx);                          /* the producer decodes into this buffer */
            for (size_t i = 0; i < in_bytes; ++i) slot[i] = (uint8_t)((i * 7 + (size_t)submitted * 31) & 255);
            CHECK(vh_ring_submit_u8(ctx, NULL, batch), ctx);                   /* in place: no extra host copy */
            ++submitted;
        } else {
            CHECK(vh_ring_collect(ctx, logits, &n), ctx);                      /* FIFO; serves both kinds of ring */
            report(logits, n, cfg.classes, collected++);
        }
    }
    free(logits);
    vh_ring_destroy(ctx);
    vh_destroy(ctx);
    return 0;
}
