/* classify_frames.c — frames of any size through the C ABI from plain C: the frames ring, resize + crop + normalisation on the GPU.
 *
 *   gcc -std=c99 -O2 -I include examples/classify_frames.c -L vit-fpga_amd -lvithip -Wl,-rpath,$PWD/vit-fpga_amd -o classify_frames
 *   ./classify_frames [--yuy2 | --bgra] [weights.vhblob | -] [batch] [submits] [height] [width]
 *
 * A producer (decoder, camera) writes each batch of height x width x 3 frames straight into the pinned buffer of the next slot and
 * says where they are (vh_frame: offset, size, row stride) and which box of each to keep; here a counter pattern stands in for it
 * and the box is the centred square of 0.875 x the short side -- torchvision's Resize(256) + CenterCrop(224).  The box is
 * resampled to image_size x image_size with the antialiased triangle filter (vithip.h, "8-bit frames") and each resulting byte p
 * of channel c enters the model as fmaf((float)p, scale[c], shift[c]).  Without a file the weights are the seeded synthetic ones.
 * --yuy2: the producer is a UVC webcam or a capture card instead and writes packed 4:2:2 frames (Y0 U Y1 V, 2 bytes per pixel;
 * vithip.h, "Packed 4:2:2 frames"): the same ring, vh_frame_yuy2 descriptors and vh_ring_submit_frames_yuy2; the colour matrix is
 * the context's (vh_set_frame_colour; default BT.709 limited range, left-sited chroma).
 * --bgra: the producer is OpenCV, a screen grabber or a GPU colour converter and writes B G R A pixels (4 bytes per pixel; vithip.h,
 * "Packed 4:4:4 frames"): vh_frame_bgra descriptors and vh_ring_submit_frames_bgra; no swizzle to tight RGB on the CPU, no matrix. */
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

static void report(const float* logits, int n, int classes, int submit) {
    for (int b = 0; b < n; ++b) {
        int best = 0;
        for (int c = 1; c < classes; ++c)
            if (logits[(size_t)b * classes + c] > logits[(size_t)b * classes + best]) best = c;
        printf("batch %d frame %d: class %d (logit %.4f)\n", submit, b, best, logits[(size_t)b * classes + best]);
    }
}

int main(int argc, char** argv) {
    const int yuy2 = argc > 1 && strcmp(argv[1], "--yuy2") == 0;
    const int bgra = argc > 1 && strcmp(argv[1], "--bgra") == 0;
    if (yuy2 || bgra) { --argc; ++argv; }
    const char* path = (argc > 1 && strcmp(argv[1], "-") != 0) ? argv[1] : NULL;
    const int batch = argc > 2 ? atoi(argv[2]) : 8;
    const int submits = argc > 3 ? atoi(argv[3]) : 6;
    const int height = argc > 4 ? atoi(argv[4]) : 360;
    const int width = argc > 5 ? atoi(argv[5]) : 480;
    const int slots = 3;
    vh_config cfg = {224, 16, 3, 768, 12, 3072, 12, 1000, VH_DTYPE_BF16, 0, 1e-6f, 0};
    if (path) CHECK(vh_blob_file_config(path, &cfg), NULL);   /* model shape from the file's header */
    cfg.max_batch = batch;
    if (cfg.channels != 3 || batch < 1 || height < 1 || width < 1) { fprintf(stderr, "this example takes 3-channel frames\n"); return 1; }
    vh_ctx* ctx = NULL;
    CHECK(vh_create(&cfg, 0, &ctx), NULL);
    if (path) CHECK(vh_load_weights_file(ctx, path), ctx);
    else CHECK(vh_init_weights_seeded(ctx, 0), ctx);

    /* (p / 255 - mean) / std  =  p * 1 / (255 std) + (-mean / std) */
    const double mean[3] = {0.485, 0.456, 0.406}, std[3] = {0.229, 0.224, 0.225};
    float scale[3], shift[3];
    for (int c = 0; c < 3; ++c) { scale[c] = (float)(1.0 / (255.0 * std[c])); shift[c] = (float)(-mean[c] / std[c]); }
    CHECK(vh_set_input_norm(ctx, scale, shift), ctx);

    /* one descriptor per frame of a batch: back to back in the slot, unpadded rows, the 0.875 centre square */
    const int row_bytes = yuy2 ? 4 * ((width + 1) / 2) : bgra ? width * 4 : width * 3; /* a YUY2 row: (width + 1) / 2 macropixels of 4 bytes */
    const size_t frame_bytes = (size_t)height * row_bytes, slot_bytes = frame_bytes * batch;
    const float side = 0.875f * (float)(height < width ? height : width);
    vh_frame* desc = (vh_frame*)malloc((size_t)batch * sizeof(vh_frame));
    vh_frame_yuy2* desc422 = (vh_frame_yuy2*)malloc((size_t)batch * sizeof(vh_frame_yuy2));
    vh_frame_bgra* desc444 = (vh_frame_bgra*)malloc((size_t)batch * sizeof(vh_frame_bgra));
    float* logits = (float*)malloc((size_t)batch * cfg.classes * sizeof(float));
    for (int b = 0; b < batch; ++b) {
        desc[b].offset = (uint64_t)b * frame_bytes;
        desc[b].height = height;
        desc[b].width = width;
        desc[b].row_stride = row_bytes;
        desc[b].box[0] = ((float)width - side) / 2;
        desc[b].box[1] = ((float)height - side) / 2;
        desc[b].box[2] = desc[b].box[0] + side;
        desc[b].box[3] = desc[b].box[1] + side;
        desc422[b].offset = desc[b].offset;
        desc422[b].height = height;
        desc422[b].width = width;
        desc422[b].row_stride = row_bytes;
        desc422[b].layout = VH_422_YUYV;                                           /* V4L2_PIX_FMT_YUYV; a DeckLink card: VH_422_UYVY */
        memcpy(desc422[b].box, desc[b].box, sizeof desc[b].box);
        desc444[b].offset = desc[b].offset;
        desc444[b].height = height;
        desc444[b].width = width;
        desc444[b].row_stride = row_bytes;
        desc444[b].layout = VH_444_BGRA;                                           /* cv::Mat of CV_8UC3: VH_444_BGR, row_stride = mat.step */
        memcpy(desc444[b].box, desc[b].box, sizeof desc[b].box);
    }
    CHECK(vh_ring_create_frames(ctx, slots, batch, slot_bytes), ctx);
    int submitted = 0, collected = 0, n = 0, free_slots = 0;
    while (collected < submits) {
        CHECK(vh_ring_free_slots(ctx, &free_slots), ctx);
        if (submitted < submits && free_slots > 0) {
            uint8_t* slot = NULL;
            size_t capacity = 0;
            CHECK(vh_ring_input_frames(ctx, &slot, &capacity), ctx);              /* the producer decodes into this buffer */
            for (size_t i = 0; i < slot_bytes && i < capacity; ++i) slot[i] = (uint8_t)((i * 7 + (size_t)submitted * 31) & 255);
            if (bgra) CHECK(vh_ring_submit_frames_bgra(ctx, NULL, slot_bytes, desc444, batch), ctx);
            else if (yuy2) CHECK(vh_ring_submit_frames_yuy2(ctx, NULL, slot_bytes, desc422, batch), ctx);
            else CHECK(vh_ring_submit_frames(ctx, NULL, slot_bytes, desc, batch), ctx); /* in place; desc may be reused at once */
            ++submitted;
        } else {
            CHECK(vh_ring_collect(ctx, logits, &n), ctx);                          /* FIFO; serves every kind of ring */
            report(logits, n, cfg.classes, collected++);
        }
    }
    free(logits);
    free(desc444);
    free(desc422);
    free(desc);
    vh_ring_destroy(ctx);
    vh_destroy(ctx);
    return 0;
}
