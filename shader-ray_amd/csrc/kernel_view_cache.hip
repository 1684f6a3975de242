// kernel_view_cache.hip -- the prepass that fills one entry of a scene's view cache (view_cache.h): for every pixel
// of a whole one-sample frame, at its row-major output index,
//   rays  the primary ray's world-space direction, by uniform_driver.h's primary_direction -- the function the frame kernels call;
//   sky   what the frame kernels store for a pixel whose primary ray leaves the scene: the environment lookup with its
//         outside_acos_is_nan rule, 0 + 1 * sky (trace()'s accumulated + modulation * sky with no bounce made), the tone map
//         if the frame asks for it, alpha 1 -- trace_common.h's environment and filmic and the driver's own expressions.
// Neither depends on the object, the light or the material.  The frame kernels' bits and these are the same bits because the
// source is the same and every operation in it is one correctly rounded IEEE operation (see primary_direction); the two
// functions' wave-uniform branches (exact_div.h's ranges, the environment's texel wrap) give a lane the same result on either
// side, so it does not matter that a wave here is 64 consecutive pixels of a row and there an 8x8 tile.
#include "launch.h"
#include "exact_div.h"
#include "uniform_driver.h"

namespace shray {

constexpr int kViewCacheBlock = 256;

__global__ void __launch_bounds__(kViewCacheBlock) view_cache_kernel(SceneView sc, const FrameView *__restrict__ frames, float *__restrict__ rays,
                                                                     float4 *__restrict__ sky)
{
    const FrameView &fr = frames[0];
    const size_t pixels = (size_t)fr.width * (size_t)fr.height;
    const size_t index = (size_t)blockIdx.x * kViewCacheBlock + threadIdx.x;   // = py * width + px, the frame kernels' out_index
    if (index >= pixels)
        return;
    const int px = (int)(index % (size_t)fr.width), py = (int)(index / (size_t)fr.width);
    const SharedDivisor by_width = shared_divisor((float)fr.width), by_height = shared_divisor((float)fr.height);
    const V3 D = primary_direction(fr, px, py, 0, 1.0f, by_width, by_height, eye_ray_in_range(fr));
    rays[3u * index] = D.x;
    rays[3u * index + 1u] = D.y;
    rays[3u * index + 2u] = D.z;
    // the driver's statements for a sample whose first traversal found nothing, in its order
    const V3 radiance = mk(0, 0, 0) + mk(1, 1, 1) * environment(sc, D);
    V3 result = radiance;
    if (fr.tonemap)
        result = mk(filmic(result.x), filmic(result.y), filmic(result.z));
    sky[index] = make_float4(result.x, result.y, result.z, 1.0f);
}

hipError_t launch_view_cache(const SceneView &sc, const FrameView *d_frame, const FrameView &fr, float *rays, float *sky, hipStream_t stream)
{
    const size_t pixels = (size_t)fr.width * (size_t)fr.height;
    const dim3 grid((unsigned int)((pixels + kViewCacheBlock - 1) / kViewCacheBlock)), block(kViewCacheBlock);
    hipLaunchKernelGGL(view_cache_kernel, grid, block, 0, stream, sc, d_frame, rays, reinterpret_cast<float4 *>(sky));
    return hipGetLastError();
}

}   // namespace shray
