// ActorCutMix composite of a batch's ActorCutMix clips in one launch (the actor_cut_mix branch of
// ActorCutMixDataset.prepare_train_frames, libs/loader/actor_cut_mix_loader.py:117-164).
//
// Per clip the reference runs, on every frame already resized to the 256 scale (Resize(-1, 256)):
//   actor (action_pipeline :86-96): FlipWithBox -> ResizeWithBox((224, 224), keep_ratio=False) -> BuildHumanMask -> SceneCutOut(127)
//   scene (scene_pipeline :74-83):  FlipWithBox -> ResizeWithBox((224, 224), keep_ratio=False) -> ActorCutOut(127)
//   actor * mask + scene * (1 - mask) per frame (:143-149), foreground_ratio = sum(mask) / (T*H*W) (:154-164), Normalize.
// Here each output pixel is produced once: the mask test against the actor's boxes of that frame (BuildHumanMask: every pixel
// when the clip has no box in any frame, libs/pipelines/box.py:184-189), then the flipped + resized actor pixel inside the mask,
// 127 inside one of the scene's own boxes (ActorCutOut, box.py:143-154), else the flipped + resized scene pixel; the result is
// normalised as bdv_crop_normalize_u8 does.  SceneCutOut (box.py:93-108) paints 127 exactly where the mask is 0, which the
// composite then replaces by the scene: it never reaches the output and is not computed.
//
// The flip + resize reads the frame mirrored (resize_pixel<true>: the taps of np.flip(frame, 1), the column index mirrored on the
// read), which equals resize(flip(frame)) bit for bit; flipping the resized output would not (cv::resize's x-axis edge handling is
// not symmetric).  The mask pixels are counted per clip: a wave reduction and one integer atomic per wave, so the count does not
// depend on the order the waves finish in.  Byte work, no MFMA; the fp32 output writes are most of its
// traffic (its limiter is not measured: profiles/r04_actor_cut_mix.txt).
#include <vector>

#include "common.h"
#include "loader_pieces.h"
#include "resize_linear.h"

namespace {

constexpr int ACM_CLIP_INTS = 5;   // out_row, actor_row, actor_flip, scene_row (-1: not read), scene_flip

struct AcmArgs {
  const uint8_t* actor;            // (n_actor, T, Ha, Wa, 3)
  const uint8_t* scene;            // (n_scene, T, Hs, Ws, 3)
  const int32_t* clips;            // nclips x ACM_CLIP_INTS
  const int32_t* aoff;             // nclips*T + 1: actor boxes of frame f are [aoff[f], aoff[f+1])
  const int32_t* soff;             // nclips*T + 1: scene boxes
  const int32_t* abox;             // x0 y0 x1 y1 in the Hd x Wd output frame
  const int32_t* sbox;
  float* out;                      // (B_out, T, 3, Hd, Wd)
  int32_t* counts;                 // (nclips) mask pixels, zeroed by the launcher
  int T, Ha, Wa, Hs, Ws, Hd, Wd;
  ClipNorm norm;
};

// numpy slice semantics img[y0:y1, x0:x1] for 0 <= coordinates <= the frame size (validated on the host): an inverted box is empty
__device__ __forceinline__ bool in_any_box(const int32_t* box, int b0, int b1, int x, int y) {
  bool in = false;
  for (int b = b0; b < b1; ++b) {
    const int32_t* q = box + 4 * b;
    in |= x >= q[0] && x < q[2] && y >= q[1] && y < q[3];
  }
  return in;
}

__device__ __forceinline__ ResizeBox frame_box(const uint8_t* src, int frame, int Hs, int Ws, int Hd, int Wd) {
  return resize_box(src + (size_t)frame * Hs * Ws * 3, (size_t)Ws * 3, Ws, Hs, Hd, Wd);
}

// grid (pixel groups of one frame, nclips*T), 256 threads; four consecutive output pixels per thread
__global__ __launch_bounds__(256) void actor_cut_mix_kernel(const AcmArgs a) {
  const unsigned npix = (unsigned)a.Hd * (unsigned)a.Wd;
  const unsigned p0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
  const int f = blockIdx.y, clip = f / a.T, t = f - clip * a.T;
  const int32_t* ct = a.clips + ACM_CLIP_INTS * clip;
  int cnt = 0;
  if (p0 < npix) {
    const int out_row = ct[0], actor_row = ct[1], actor_flip = ct[2], scene_row = ct[3], scene_flip = ct[4];
    const bool whole = a.aoff[clip * a.T] == a.aoff[clip * a.T + a.T];        // no actor box in the clip: the mask is all ones
    const int ab0 = a.aoff[f], ab1 = a.aoff[f + 1], sb0 = a.soff[f], sb1 = a.soff[f + 1];
    const ResizeBox ra = frame_box(a.actor, actor_row * a.T + t, a.Ha, a.Wa, a.Hd, a.Wd);
    // scene_row < 0 only for a clip without actor boxes (checked on the host): every pixel is then the actor's
    const ResizeBox rs = frame_box(a.scene, (scene_row < 0 ? 0 : scene_row) * a.T + t, a.Hs, a.Ws, a.Hd, a.Wd);
    ResizeGroup g = resize_group(p0, npix, a.Wd);
    const int cnt4 = g.cnt;
    float v[3][4];
#pragma unroll
    for (int k = 0; k < 4; ++k, g.next(a.Wd)) {
      unsigned px = 0;
      if (k < cnt4) {
        const bool m = whole || in_any_box(a.abox, ab0, ab1, g.dx, g.dy);
        if (m)
          px = actor_flip ? resize_pixel<true>(ra, g.dx, g.dy) : resize_pixel<false>(ra, g.dx, g.dy);
        else if (in_any_box(a.sbox, sb0, sb1, g.dx, g.dy))
          px = 0x7F7F7Fu;                                                       // ActorCutOut(fill_color=127)
        else
          px = scene_flip ? resize_pixel<true>(rs, g.dx, g.dy) : resize_pixel<false>(rs, g.dx, g.dy);
        cnt += m;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c][k] = normalize_u8((uint8_t)(px >> (8 * c)), a.norm.mean[c], a.norm.inv_std[c]);
    }
    float* o = a.out + ((size_t)out_row * a.T + t) * 3 * npix + p0;
    if (cnt4 == 4 && (npix & 3u) == 0u) {
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + (size_t)c * npix) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
    } else {
      for (int c = 0; c < 3; ++c)
        for (int k = 0; k < cnt4; ++k) o[(size_t)c * npix + k] = v[c][k];
    }
  }
  // every lane takes part in the reduction (no early return above)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if ((threadIdx.x & 63u) == 0u && cnt != 0) atomicAdd(a.counts + clip, cnt);
}

}  // namespace

extern "C" int bdv_actor_cut_mix_u8(const uint8_t* actor, int n_actor, int Ha, int Wa, const uint8_t* scene, int n_scene, int Hs, int Ws,
                                    const int32_t* plan, const int32_t* plan_host, int64_t plan_len, int nclips, int T, int Hd, int Wd,
                                    const float mean[3], const float inv_std[3], float* out, int B_out, int32_t* counts, void* stream) {
  BDV_REQUIRE(actor && plan && plan_host && mean && inv_std && out && counts, "bdv_actor_cut_mix_u8: null pointer");
  BDV_REQUIRE(nclips > 0 && T > 0 && Hd > 0 && Wd > 0 && B_out > 0 && n_actor > 0 && Ha > 0 && Wa > 0,
              "bdv_actor_cut_mix_u8: bad shape nclips=%d T=%d %dx%d B_out=%d actor %d x %dx%d", nclips, T, Hd, Wd, B_out, n_actor, Ha, Wa);
  BDV_REQUIRE(n_scene >= 0 && (n_scene == 0 || (scene && Hs > 0 && Ws > 0)), "bdv_actor_cut_mix_u8: bad scene frames n=%d %dx%d", n_scene, Hs, Ws);
  BDV_REQUIRE((long long)nclips * T <= 65535, "bdv_actor_cut_mix_u8: %lld frames exceed one grid dimension", (long long)nclips * T);
  BDV_REQUIRE((long long)Hd * Wd < (1ll << 30) && (long long)Ha * Wa < (1ll << 29) && (long long)Hs * Ws < (1ll << 29),
              "bdv_actor_cut_mix_u8: frame too large");
  BDV_REQUIRE((((uintptr_t)out) & 15) == 0, "bdv_actor_cut_mix_u8: out must be 16-byte aligned");
  // the plan is read by the kernel on the device; every index it holds is checked here, on the host copy, before the launch
  const long long F = (long long)nclips * T;
  const long long head = (long long)ACM_CLIP_INTS * nclips + 2 * (F + 1);
  BDV_REQUIRE(plan_len >= head, "bdv_actor_cut_mix_u8: plan of %lld ints is shorter than its %lld-int head", (long long)plan_len, head);
  const int32_t* clips = plan_host;
  const int32_t* offs[2] = {plan_host + ACM_CLIP_INTS * nclips, plan_host + ACM_CLIP_INTS * nclips + F + 1};
  for (int s = 0; s < 2; ++s) {
    BDV_REQUIRE(offs[s][0] == 0, "bdv_actor_cut_mix_u8: %s box offsets must start at 0", s ? "scene" : "actor");
    for (long long f = 0; f < F; ++f) {
      const long long n = (long long)offs[s][f + 1] - offs[s][f];
      BDV_REQUIRE(n >= 0 && n <= BDV_ACM_MAX_BOXES, "bdv_actor_cut_mix_u8: %s frame %lld has %lld boxes (0..%d)", s ? "scene" : "actor", f, n,
                  BDV_ACM_MAX_BOXES);
    }
  }
  const long long na = offs[0][F], ns = offs[1][F];
  BDV_REQUIRE(plan_len == head + 4 * (na + ns), "bdv_actor_cut_mix_u8: plan of %lld ints, its offsets need %lld", (long long)plan_len,
              head + 4 * (na + ns));
  const int32_t* boxes = plan_host + head;
  for (long long i = 0; i < na + ns; ++i) {
    const int32_t* q = boxes + 4 * i;
    BDV_REQUIRE(q[0] >= 0 && q[0] <= Wd && q[2] >= 0 && q[2] <= Wd && q[1] >= 0 && q[1] <= Hd && q[3] >= 0 && q[3] <= Hd,
                "bdv_actor_cut_mix_u8: %s box %lld = (%d, %d, %d, %d) leaves the %d x %d frame", i < na ? "actor" : "scene", i < na ? i : i - na,
                q[0], q[1], q[2], q[3], Wd, Hd);
  }
  std::vector<char> used(B_out, 0);
  for (int c = 0; c < nclips; ++c) {
    const int32_t* q = clips + ACM_CLIP_INTS * c;
    BDV_REQUIRE(q[0] >= 0 && q[0] < B_out && !used[q[0]], "bdv_actor_cut_mix_u8: clip %d: output row %d out of range [0, %d) or repeated", c, q[0], B_out);
    used[q[0]] = 1;
    BDV_REQUIRE(q[1] >= 0 && q[1] < n_actor, "bdv_actor_cut_mix_u8: clip %d: actor row %d out of range [0, %d)", c, q[1], n_actor);
    BDV_REQUIRE((q[2] == 0 || q[2] == 1) && (q[4] == 0 || q[4] == 1), "bdv_actor_cut_mix_u8: clip %d: flips must be 0 or 1", c);
    const bool whole = offs[0][(long long)c * T] == offs[0][(long long)(c + 1) * T];
    BDV_REQUIRE((whole && q[3] == -1) || (q[3] >= 0 && q[3] < n_scene),
                "bdv_actor_cut_mix_u8: clip %d: scene row %d out of range [0, %d) (-1 only for a clip without actor boxes)", c, q[3], n_scene);
  }
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)nclips * sizeof(int32_t), st);
  if (e != hipSuccess) {
    bdv_set_error("bdv_actor_cut_mix_u8: memset failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  AcmArgs a;
  a.actor = actor;
  a.scene = n_scene > 0 ? scene : actor;   // never read without a scene row; any valid pointer
  a.clips = plan;
  a.aoff = plan + ACM_CLIP_INTS * nclips;
  a.soff = a.aoff + F + 1;
  a.abox = plan + head;
  a.sbox = a.abox + 4 * na;
  a.out = out;
  a.counts = counts;
  a.T = T;
  a.Ha = Ha;
  a.Wa = Wa;
  a.Hs = n_scene > 0 ? Hs : Ha;
  a.Ws = n_scene > 0 ? Ws : Wa;
  a.Hd = Hd;
  a.Wd = Wd;
  a.norm = clip_norm(mean, inv_std);
  const unsigned groups = ((unsigned)Hd * (unsigned)Wd + 3u) / 4u;
  hipLaunchKernelGGL(actor_cut_mix_kernel, dim3((groups + 255u) / 256u, (unsigned)F), dim3(256), 0, st, a);
  BDV_LAUNCH_CHECK("bdv_actor_cut_mix_u8");
  return BDV_OK;
}
