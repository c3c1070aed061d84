// store_pack.hip — the passes of ws_store_pack and ws_store_unpack (include/warpsense_hip.h; the format is in ws_pack.h, the host
// flow in api_pack.hip): the chunks the host lists into brick class maps and one payload stream, and back.
//
// Every pass walks a chunk the same way.  A wave takes one BRICK COLUMN: fixed (x >> 3, y >> 3), all eight z >> 3, and walks its 64
// (x, y) columns of the chunk with lane = z: every chunk access is one 256-byte line, and the eight lanes of a group (lane >> 3) are
// one brick.  A workgroup is four brick columns, 16 workgroups a chunk (blockIdx.x), blockIdx.y strides over the chunks.
//   classify: a lane carries "differs from fill" and "differs from the brick's word 0" over the 64 columns; two ballots give the
//     eight class codes of the wave, 16 bits of the class map, stored as one half word.  The counts of a chunk are one integer add
//     per workgroup (the headers are zeroed in front of the pass).  No floating point.
//   scan: one workgroup carries a 64-bit running sum over the chunks' payload sizes.
//   emit: the workgroup turns the chunk's class map into the 512 brick offsets in LDS.  A dense brick's 512 words are contiguous in
//     the payload but lie in 64 different lines of the chunk: written straight from the lanes that read them they are 32-byte runs
//     (WS_PACK_EMIT_DIRECT); by default a wave stages four x planes of its brick column in LDS (8 bricks x 256 words, the brick
//     stride padded to 264 words: the eight groups of a store hit eight different banks of every 32-lane half) and writes each
//     dense brick's 256 words as four 256-byte runs.  Payload indices are 64-bit and bounded by the buffer's capacity.
//   unpack: the mirror image.  The lanes pick fill, the brick's one word or their own payload word and write whole lines.
#include "ws_device.h"
#include "ws_pack.h"

namespace ws
{
namespace
{
constexpr uint32_t PACK_WG = 256, PACK_PARTS = 16; // threads of a workgroup; workgroups of a chunk (four brick columns each)
constexpr uint32_t PACK_STAGE_STRIDE = 264;       // words of a staged half brick (256) + 8
static_assert(PACK_WG == PACK_OFFSETS_WG, "pack_brick_offsets (ws_pack.h) takes two bricks per thread of the emit and unpack workgroups");

struct PackArgs
{
  const StoreRaySlot *table; // [n] {cx, cy, cz, slot}, ascending keys
  uint32_t n;
  uint32_t *const *segs;     // base pointers of the store's segments
  uint32_t seg_shift;
  uint32_t fill;
  uint32_t *headers;         // [n][PACK_HDR]
  uint32_t *payload;
  uint64_t cap;              // words of `payload`
};

struct UnpackArgs
{
  const uint32_t *headers;   // [n][PACK_HDR]
  const uint32_t *slots;     // [n]
  uint32_t n;
  uint32_t *const *segs;
  uint32_t seg_shift;
  uint32_t fill;
  const uint32_t *payload;
};

__device__ __forceinline__ uint32_t *pack_chunk_ptr(uint32_t *const *segs, uint32_t seg_shift, uint32_t slot)
{
  return segs[slot >> seg_shift] + (size_t)(slot & ((1u << seg_shift) - 1u)) * (size_t)STORE_CHUNK_WORDS;
}

// the first word of this wave's brick column in a chunk, for this lane: column (x, y) of it is at + x * 4096 + y * 64
__device__ __forceinline__ uint32_t pack_column_at(uint32_t bx, uint32_t by, uint32_t lane) { return bx * 8u * 4096u + by * 8u * 64u + lane; }

__global__ __launch_bounds__(PACK_WG) void pack_classify_kernel(PackArgs a)
{
  __shared__ uint32_t cnt[2][4];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t bx = blockIdx.x >> 1, by = (blockIdx.x & 1u) * 4u + wave;
  for (uint32_t c = blockIdx.y; c < a.n; c += gridDim.y)
  {
    const StoreRaySlot e = a.table[c];
    const uint32_t *col = pack_chunk_ptr(a.segs, a.seg_shift, e.slot) + pack_column_at(bx, by, lane);
    uint32_t *hdr = a.headers + (size_t)c * PACK_HDR;
    bool d_fill = false, d_w0 = false;
    uint32_t w0 = 0;
    for (uint32_t x = 0; x < 8u; ++x)
    {
      uint32_t w[8];
#pragma unroll
      for (uint32_t y = 0; y < 8u; ++y) w[y] = col[x * 4096u + y * 64u];
      if (x == 0u) w0 = __shfl(w[0], (int)(lane & 56u), 64); // the brick's word 0: column (0, 0), z & 7 == 0
#pragma unroll
      for (uint32_t y = 0; y < 8u; ++y) d_fill |= w[y] != a.fill, d_w0 |= w[y] != w0;
    }
    const unsigned long long m_fill = __ballot(d_fill), m_w0 = __ballot(d_w0);
    // lane g < 8 holds the code of brick g of the column
    uint32_t code = 0;
    if (lane < 8u) code = pack_class(((m_fill >> (8u * lane)) & 0xffull) != 0ull, ((m_w0 >> (8u * lane)) & 0xffull) != 0ull);
    const uint32_t n_uniform = (uint32_t)__popcll(__ballot(code == PACK_UNIFORM)), n_dense = (uint32_t)__popcll(__ballot(code == PACK_DENSE));
    uint32_t bits = lane < 8u ? code << (2u * lane) : 0u;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) bits |= __shfl_xor(bits, o, 64);
    if (lane == 0u)
    {
      // the column's first brick is (bx * 8 + by) * 8: its eight codes are one half of a map word
      reinterpret_cast<uint16_t *>(hdr + PACK_HDR_MAP)[bx * 8u + by] = (uint16_t)bits;
      cnt[0][wave] = n_uniform, cnt[1][wave] = n_dense;
    }
    __syncthreads();
    if (threadIdx.x == 0u)
    {
      const uint32_t u = cnt[0][0] + cnt[0][1] + cnt[0][2] + cnt[0][3], d = cnt[1][0] + cnt[1][1] + cnt[1][2] + cnt[1][3];
      if (u) atomicAdd(hdr + PACK_HDR_UNIFORM, u);
      if (d) atomicAdd(hdr + PACK_HDR_DENSE, d);
      if (blockIdx.x == 0u) hdr[PACK_HDR_KEY] = (uint32_t)e.cx, hdr[PACK_HDR_KEY + 1] = (uint32_t)e.cy, hdr[PACK_HDR_KEY + 2] = (uint32_t)e.cz;
    }
    __syncthreads();
  }
}

// one workgroup: the exclusive 64-bit scan of the chunks' payload words into their headers; sums[3]: payload words, uniform bricks,
// dense bricks of the call (pack_scan, ws_pack.h)
__global__ __launch_bounds__(PACK_SCAN_WG) void pack_scan_kernel(uint32_t *headers, uint32_t n, unsigned long long *sums)
{
  __shared__ unsigned long long wtot[PACK_SCAN_WG / 64], red[2][PACK_SCAN_WG / 64];
  pack_scan(headers, n, sums, wtot, red);
}

template <bool DIRECT>
__global__ __launch_bounds__(PACK_WG) void pack_emit_kernel(PackArgs a)
{
  __shared__ uint32_t map[32], off[PACK_BRICKS], part[4];
  __shared__ uint32_t stage[DIRECT ? 1 : 4][DIRECT ? 1 : 8][DIRECT ? 1 : PACK_STAGE_STRIDE];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t bx = blockIdx.x >> 1, by = (blockIdx.x & 1u) * 4u + wave;
  const uint32_t b0 = (bx * 8u + by) * 8u, g = lane >> 3, z7 = lane & 7u;
  for (uint32_t c = blockIdx.y; c < a.n; c += gridDim.y)
  {
    const StoreRaySlot e = a.table[c];
    const uint32_t *col = pack_chunk_ptr(a.segs, a.seg_shift, e.slot) + pack_column_at(bx, by, lane);
    const uint32_t *hdr = a.headers + (size_t)c * PACK_HDR;
    pack_brick_offsets(hdr, map, off, part);
    const uint64_t first = pack_chunk_first(hdr);
    const uint32_t code = pack_map_code(map, b0 + g);
    const uint64_t mine = first + off[b0 + g]; // the first payload word of this lane's brick
    const bool any = __ballot(code != PACK_DEFAULT) != 0ull; // (a column of default bricks is not read; its wave still meets the barriers)
    for (uint32_t x = 0; x < 8u; ++x)
    {
      uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (any)
      {
#pragma unroll
        for (uint32_t y = 0; y < 8u; ++y) w[y] = col[x * 4096u + y * 64u];
        if (x == 0u && z7 == 0u && code == PACK_UNIFORM && mine < a.cap) a.payload[mine] = w[0];
      }
      if (DIRECT)
      {
#pragma unroll
        for (uint32_t y = 0; y < 8u; ++y)
        {
          const uint64_t at = mine + (x * 64u + y * 8u + z7);
          if (code == PACK_DENSE && at < a.cap) a.payload[at] = w[y];
        }
      }
      else
      {
#pragma unroll
        for (uint32_t y = 0; y < 8u; ++y) stage[wave][g][(x & 3u) * 64u + y * 8u + z7] = w[y];
        if ((x & 3u) == 3u) // four x planes are staged: 256 consecutive words of each brick
        {
          __syncthreads();
          for (uint32_t k = 0; k < 8u && any; ++k)
          {
            if (pack_map_code(map, b0 + k) != PACK_DENSE) continue; // (uniform over the wave)
            const uint64_t at0 = first + off[b0 + k] + (x >> 2) * 256u + lane;
#pragma unroll
            for (uint32_t r = 0; r < 4u; ++r)
              if (at0 + r * 64u < a.cap) a.payload[at0 + r * 64u] = stage[wave][k][r * 64u + lane];
          }
          __syncthreads();
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(PACK_WG) void unpack_kernel(UnpackArgs a)
{
  __shared__ uint32_t map[32], off[PACK_BRICKS], part[4];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t bx = blockIdx.x >> 1, by = (blockIdx.x & 1u) * 4u + wave;
  const uint32_t b0 = (bx * 8u + by) * 8u, g = lane >> 3, z7 = lane & 7u;
  for (uint32_t c = blockIdx.y; c < a.n; c += gridDim.y)
  {
    const uint32_t *hdr = a.headers + (size_t)c * PACK_HDR;
    uint32_t *col = pack_chunk_ptr(a.segs, a.seg_shift, a.slots[c]) + pack_column_at(bx, by, lane);
    pack_brick_offsets(hdr, map, off, part);
    const uint32_t code = pack_map_code(map, b0 + g);
    const uint32_t *mine = a.payload + (pack_chunk_first(hdr) + off[b0 + g]);
    uint32_t flat = a.fill;
    if (code == PACK_UNIFORM) flat = mine[0];
    for (uint32_t x = 0; x < 8u; ++x)
    {
      uint32_t w[8];
#pragma unroll
      for (uint32_t y = 0; y < 8u; ++y) w[y] = code == PACK_DENSE ? mine[x * 64u + y * 8u + z7] : flat;
#pragma unroll
      for (uint32_t y = 0; y < 8u; ++y) col[x * 4096u + y * 64u] = w[y];
    }
    __syncthreads();
  }
}
} // namespace

int launch_store_pack_count(ws_store *st, ws_store::Pack &q, const void *table_dev, size_t n)
{
  hipStream_t s = st->ctx->stream;
  PackArgs a;
  a.table = static_cast<const StoreRaySlot *>(table_dev);
  a.n = (uint32_t)n;
  a.segs = st->seg_tab.as<uint32_t *>();
  a.seg_shift = st->seg_shift;
  a.fill = st->fill;
  a.headers = q.headers.as<uint32_t>();
  a.payload = nullptr;
  a.cap = 0;
  q.timer.mark(0, s);
  WS_HIP(hipMemsetAsync(a.headers, 0, n * PACK_HDR * sizeof(uint32_t), s)); // the counts are added, word 7 stays 0
  hipLaunchKernelGGL(pack_classify_kernel, dim3(PACK_PARTS, (unsigned)std::min<size_t>(n, 65535)), dim3(PACK_WG), 0, s, a);
  WS_HIP(hipGetLastError());
  q.timer.mark(1, s);
  hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(PACK_SCAN_WG), 0, s, a.headers, a.n, q.words.dev);
  WS_HIP(hipGetLastError());
  q.timer.mark(2, s);
  return WS_OK;
}

int launch_store_pack_emit(ws_store *st, ws_store::Pack &q, const void *table_dev, size_t n, bool direct, uint64_t cap)
{
  hipStream_t s = st->ctx->stream;
  PackArgs a;
  a.table = static_cast<const StoreRaySlot *>(table_dev);
  a.n = (uint32_t)n;
  a.segs = st->seg_tab.as<uint32_t *>();
  a.seg_shift = st->seg_shift;
  a.fill = st->fill;
  a.headers = q.headers.as<uint32_t>();
  a.payload = q.payload.as<uint32_t>();
  a.cap = cap;
  const dim3 grid(PACK_PARTS, (unsigned)std::min<size_t>(n, 65535));
  q.timer.mark(3, s);
  if (direct)
    hipLaunchKernelGGL((pack_emit_kernel<true>), grid, dim3(PACK_WG), 0, s, a);
  else
    hipLaunchKernelGGL((pack_emit_kernel<false>), grid, dim3(PACK_WG), 0, s, a);
  WS_HIP(hipGetLastError());
  q.timer.mark(4, s);
  return WS_OK;
}

int launch_store_unpack(ws_store *st, ws_store::Pack &q, const uint32_t *table_dev, size_t n, const uint32_t *payload_dev, uint32_t fill)
{
  hipStream_t s = st->ctx->stream;
  UnpackArgs a;
  a.headers = table_dev;
  a.slots = table_dev + n * PACK_HDR;
  a.n = (uint32_t)n;
  a.segs = st->seg_tab.as<uint32_t *>();
  a.seg_shift = st->seg_shift;
  a.fill = fill;
  a.payload = payload_dev;
  q.timer.mark(0, s);
  hipLaunchKernelGGL(unpack_kernel, dim3(PACK_PARTS, (unsigned)std::min<size_t>(n, 65535)), dim3(PACK_WG), 0, s, a);
  WS_HIP(hipGetLastError());
  q.timer.mark(1, s);
  return WS_OK;
}
} // namespace ws
