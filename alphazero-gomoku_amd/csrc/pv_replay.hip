// Replay-buffer gather (include/azg_pv.h azg_pv_replay_gather): training batches from a
// device-resident ring of canonical positions.  Each position is stored once as int8
// stones (0 empty, 1 side to move, 2 opponent) + fp32 pi + fp32 z; a batch element is
// one of its dihedral images, encoded on the fly:
//   planes  <- Gomoku.get_encoded_state (games/gomoku.py:130-150)
//   image s <- MCTS.symmetries (mcts/new_mcts_alpha.py:42-56): np.rot90 by k = s / 2
//              (counter-clockwise), then a column flip when s is odd.
// Every output value is a copy or a 0/1 constant: the result equals numpy's bit for bit.  The ring's
// slot map, sym_src_sq and the entry points' argument checks are pv_replay.h's.
#include "pv_replay.h"

namespace azg {

// One 256-thread workgroup per sample; thread j < 225 owns output square j (stores
// coalesced along j; the loads are a permutation of one 225-element row).
__global__ __launch_bounds__(256) void replay_gather_kernel(
    const int8_t* __restrict__ stones, const float* __restrict__ pis, const float* __restrict__ zs, int cap_pos,
    int head, int count, int nsym, const int64_t* __restrict__ ids, float* __restrict__ x,
    float* __restrict__ pi_out, float* __restrict__ z_out)
{
    const int b = blockIdx.x;
    // an id outside [0, count * nsym) is clamped: it never reads outside the ring (as in the kernel below)
    const int64_t last = (int64_t)count * nsym - 1;
    int64_t id = ids[b];
    id = id < 0 ? 0 : (id > last ? last : id);
    const int s = (int)(id % nsym);
    const int pos = ring_slot(head, id / nsym, cap_pos);
    const int j = threadIdx.x;
    if (j < PIX) {
        const int src = sym_src_sq(j, s);
        const int8_t v = stones[(size_t)pos * PIX + src];
        float* xo = x + (size_t)b * 3 * PIX;
        xo[j] = v == 1 ? 1.f : 0.f;
        xo[PIX + j] = v == 2 ? 1.f : 0.f;
        xo[2 * PIX + j] = 1.f;
        pi_out[(size_t)b * PIX + j] = pis[(size_t)pos * PIX + src];
    }
    if (j == 0) z_out[b] = zs[pos];
}

// One per-position fp32 value per sample (the policy loss weight): the same id -> slot map,
// one thread per sample.
__global__ __launch_bounds__(256) void replay_gather_weight_kernel(
    const float* __restrict__ vals, int cap_pos, int head, int count, int nsym, const int64_t* __restrict__ ids,
    int batch, float* __restrict__ out)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    const int64_t last = (int64_t)count * nsym - 1;
    int64_t id = ids[b];
    id = id < 0 ? 0 : (id > last ? last : id);
    out[b] = vals[ring_slot(head, id / nsym, cap_pos)];
}

}  // namespace azg

extern "C" int32_t azg_pv_replay_gather(const int8_t* stones, const float* pis, const float* zs, int32_t cap_pos,
                                        int32_t head, int32_t count, int32_t nsym, const int64_t* ids, int32_t batch,
                                        float* x, float* pi_out, float* z_out, void* stream)
{
    using namespace azg;
    if (AZG_NULL_ARG(stones) || AZG_NULL_ARG(pis) || AZG_NULL_ARG(zs) || AZG_NULL_ARG(ids) || AZG_NULL_ARG(x) ||
        AZG_NULL_ARG(pi_out) || AZG_NULL_ARG(z_out))
        return 1;
    if (bad_nsym(__func__, nsym) || bad_batch(__func__, batch) || bad_ring(__func__, cap_pos, head, count)) return 1;
    hipLaunchKernelGGL(replay_gather_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, stones, pis, zs,
                       cap_pos, head, count, nsym, ids, x, pi_out, z_out);
    return launched(__func__, "launch");
}

extern "C" int32_t azg_pv_replay_gather_weight(const float* vals, int32_t cap_pos, int32_t head, int32_t count,
                                               int32_t nsym, const int64_t* ids, int32_t batch, float* out,
                                               void* stream)
{
    using namespace azg;
    if (AZG_NULL_ARG(vals) || AZG_NULL_ARG(ids) || AZG_NULL_ARG(out)) return 1;
    if (bad_nsym(__func__, nsym) || bad_batch(__func__, batch) || bad_ring(__func__, cap_pos, head, count)) return 1;
    hipLaunchKernelGGL(replay_gather_weight_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, vals, cap_pos, head, count, nsym, ids, batch, out);
    return launched(__func__, "launch");
}
