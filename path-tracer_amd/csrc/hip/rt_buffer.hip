// rt_buffer.hip — host side of libpathtracer.so: the sample buffer and its resolve.
#include "runtime.hpp"

using namespace ptrt;

extern "C" {

pt_sample_buffer* ptCreateSampleBuffer(pt_device* d, uint32_t w, uint32_t h)
{
    if (!d || w == 0 || h == 0) { SetError("bad sample buffer arguments"); return nullptr; }
    if (hipSetDevice(d->id) != hipSuccess) { SetError("hipSetDevice failed"); return nullptr; }
    pt_sample_buffer* b = new pt_sample_buffer;
    b->dev = d;
    b->width = w;
    b->height = h;
    size_t bytes = (size_t)w * h * sizeof(float4);
    // Cleared on the device's own stream and waited for: that stream is
    // non-blocking, so a clear on the null stream is not ordered before the
    // first ptWriteSampleBuffer and could land after it.
    if (hipMalloc(&b->accum, bytes) != hipSuccess || hipMemsetAsync(b->accum, 0, bytes, d->stream) != hipSuccess ||
        hipStreamSynchronize(d->stream) != hipSuccess) {
        SetError("sample buffer allocation failed (%zu bytes)", bytes);
        if (b->accum) (void)hipFree(b->accum);
        delete b;
        return nullptr;
    }
    return b;
}

void ptDestroySampleBuffer(pt_device* d, pt_sample_buffer* b)
{
    if (!b) return;
    if (d) (void)hipSetDevice(d->id);
    if (b->accum) (void)hipFree(b->accum);
    delete b;
}

int ptReadSampleBuffer(pt_device* d, pt_sample_buffer* b, float* rgba)
{
    if (!d || !b || !rgba) { SetError("null argument"); return -1; }
    return ReadBack(d, rgba, b->accum, (size_t)b->width * b->height * sizeof(float4));
}

int ptWriteSampleBuffer(pt_device* d, pt_sample_buffer* b, const float* rgba)
{
    if (!d || !b || !rgba) { SetError("null argument"); return -1; }
    return WriteThrough(d, b->accum, rgba, (size_t)b->width * b->height * sizeof(float4));
}

// RenderSampleBuffer (integrator.cpp:105-159 + resolve.glsl:112-128)
int ptRenderSampleBuffer(pt_device* d, pt_sample_buffer* b, const pt_resolve_parameters* p)
{
    if (!d || !b || !p) { SetError("null argument"); return -1; }
    if (p->ToneMappingMode > PT_TONE_MAPPING_ACES) { SetError("bad tone mapping mode %u", p->ToneMappingMode); return -1; }
    PT_HIP(hipSetDevice(d->id));
    size_t n = (size_t)b->width * b->height;
    PT_HIP(b->display.alloc(n));
    PT_HIP(b->display8.alloc(n));
    PT_TIMED(d, PT_KERNEL_RESOLVE,
             pt_launch_resolve(b->accum, (uint32_t)n, p->Brightness, p->ToneMappingMode, p->ToneMappingWhiteLevel,
                               b->display.ptr, b->display8.ptr, d->stream));
    b->resolved = true;
    return 0;
}

int ptReadResolvedImage(pt_device* d, pt_sample_buffer* b, float* rgba)
{
    if (!d || !b || !rgba) { SetError("null argument"); return -1; }
    if (!b->resolved) { SetError("sample buffer not resolved (call ptRenderSampleBuffer)"); return -1; }
    return ReadBack(d, rgba, b->display.ptr, (size_t)b->width * b->height * sizeof(float4));
}

int ptReadResolvedImageSRGB8(pt_device* d, pt_sample_buffer* b, uint8_t* rgba8)
{
    if (!d || !b || !rgba8) { SetError("null argument"); return -1; }
    if (!b->resolved) { SetError("sample buffer not resolved (call ptRenderSampleBuffer)"); return -1; }
    return ReadBack(d, rgba8, b->display8.ptr, (size_t)b->width * b->height * 4);
}

}  // extern "C"
