// Host-side launcher for decode_combine_kernel (attention_decode.hip): merges
// the split-K partials (o_part [B*Hk*nsplit, G, 128] f32, ml_part
// [B*Hk*nsplit, G, 2] f32) into out [B, Hq, 128] bf16. Shared by every decode
// attention kernel that publishes partials in that layout (kv_fp8.hip).
#pragma once

extern "C" int oa_decode_combine(void* stream, const void* o_part,
                                 const void* ml_part, void* out, int B, int Hq,
                                 int Hk, int nsplit);
