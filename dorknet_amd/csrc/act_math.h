// The four activations beyond ReLU (layers/activations.py: LeakyReLu, ReLu6, HardSwish, SiLu) for one
// fp32 element: y = act(v) and g = dy * act'(v).  DESIGN.md section 23.
//
// Every fp32 operation here is rounded once on its own (contraction is off inside each function, and
// stays off when the function is inlined into a translation unit that contracts), so the numpy float32
// twin (tests/_activation_twin.py) reproduces each result bit for bit.  Nothing calls a library: SiLu's
// exponential is restated below from + - * /, integer operations and a power of two built from the
// exponent field.
//
// The derivative at a kink is torch's (F.leaky_relu, F.relu6, F.hardswish): alpha at 0; 0 at 0 and at 6; 0 at -3
// and 1 at 3.
//
// Special values, as the rules below give them (the twin states the same):
//   NaN     y and g are NaN, except LeakyReLu's g = alpha * dy and ReLu6's g = 0 (the comparisons fail).
//   +-0     LeakyReLu y = alpha * v, g = alpha * dy; ReLu6 y = v (the zero keeps its sign), g = 0;
//           HardSwish y = (v * 3) / 6 = +-0, g = dy / 2; SiLu y = +-0, g = dy / 2.
//   +inf    y = v (ReLu6: 6), g = dy (ReLu6: 0); SiLu's g is NaN (inf * (1 - 1)).
//   -inf    LeakyReLu y = alpha * -inf, g = alpha * dy; ReLu6 y = 0, g = 0; HardSwish y = 0, g = 0 (the
//           v <= -3 branch: no -inf * 0); SiLu y = -inf, g = dy * -inf (the sigmoid is clamped at e^-80).
//   |v| large, finite (1e4): every rule is finite; SiLu takes s = 1 (v > 0) or s = e^-80 (v < 0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dk {

enum ActKind : int { kActLeaky = 0, kActRelu6 = 1, kActHardSwish = 2, kActSilu = 3, kNumActKinds = 4 };

constexpr float kActSixth = 0.16666667163372039794921875f;  // fl32(1 / 6)

// e^(-a) for a = min(|v|, 80): z in (0, 1], no overflow, no subnormal (2^-k with k <= 115).
//   k = rint(a * log2 e) by the 1.5 * 2^23 shift (two fp32 additions, round to nearest even);
//   r = (a - k * C1) - k * C2 with C1 = 0.693359375 (k * C1 exact) and C1 + C2 = ln 2: |r| <= 0.3466;
//   e^(-r) by the degree-7 Taylor polynomial in t = -r, Horner with separate multiply and add;
//   z = p * 2^-k, the power of two assembled in the exponent field (an exact scaling).
__device__ __forceinline__ float act_exp_neg_abs(float v) {
#pragma clang fp contract(off)
  float a = v < 0.f ? -v : v;
  if (!(a <= 80.f)) a = 80.f;  // (a NaN is clamped too: the result of the caller is NaN through v)
  const float shift = 12582912.f;
  const float kf = (a * 1.44269502162933349609375f + shift) - shift;
  const float r = (a - kf * 0.693359375f) - kf * -2.12194441701285541057586669921875e-4f;
  const float t = -r;
  float p = 1.98412701138295233249664306640625e-4f;     // 1 / 5040
  p = p * t + 1.388888922519981861114501953125e-3f;     // 1 / 720
  p = p * t + 8.333333767950534820556640625e-3f;        // 1 / 120
  p = p * t + 4.16666679084300994873046875e-2f;         // 1 / 24
  p = p * t + kActSixth;
  p = p * t + 0.5f;
  p = p * t + 1.0f;
  p = p * t + 1.0f;
  const int k = (int)kf;
  return p * __builtin_bit_cast(float, (uint32_t)(127 - k) << 23);
}

// s(v) = 1 / (1 + e^-v) from z = e^-|v|
__device__ __forceinline__ float act_sigmoid(float v) {
#pragma clang fp contract(off)
  const float z = act_exp_neg_abs(v);
  const float d = 1.0f + z;
  return v >= 0.f ? __fdiv_rn(1.0f, d) : __fdiv_rn(z, d);
}

__device__ __forceinline__ float act_fwd(int kind, float alpha, float v) {
#pragma clang fp contract(off)
  switch (kind) {
    case kActLeaky:
      return v > 0.f ? v : alpha * v;
    case kActRelu6: {
      const float t = v < 0.f ? 0.f : v;
      return t > 6.f ? 6.f : t;
    }
    case kActHardSwish:
      return v <= -3.f ? 0.f : (v >= 3.f ? v : (v * (v + 3.f)) * kActSixth);
    default:
      return v * act_sigmoid(v);
  }
}

// g = dy * act'(v)
__device__ __forceinline__ float act_grad(int kind, float alpha, float v, float dy) {
#pragma clang fp contract(off)
  switch (kind) {
    case kActLeaky:
      return v > 0.f ? dy : alpha * dy;
    case kActRelu6:
      return (v > 0.f && v < 6.f) ? dy : 0.f;
    case kActHardSwish:
      return v <= -3.f ? 0.f : (v >= 3.f ? dy : dy * ((2.0f * v + 3.f) * kActSixth));
    default: {
      const float s = act_sigmoid(v);
      return dy * (s * (1.0f + v * (1.0f - s)));
    }
  }
}

}  // namespace dk
