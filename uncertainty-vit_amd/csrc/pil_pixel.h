// Pillow's pixel arithmetic shared by augment.hip (ColorJitter) and randaug.hip (the ImageEnhance ops): Convert.c's rgb2l and Blend.c's
// Image.blend.  Both files are built without -ffast-math and with -ffp-contract=off: d + f * (x - d) is a float multiply, then a float add.
#pragma once

__device__ inline int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }  // Convert.c rgb2l

// Blend.c: float temp = in1 + alpha * (in2 - in1); clipped to [0, 255], truncated
__device__ inline int blend(int d, int x, float f) {
    const float t = (float)d + f * (float)(x - d);
    if (t <= 0.0f) return 0;
    if (t >= 255.0f) return 255;
    return (int)t;
}
