// lrf_planes_ragged_kernel.hip — uint8 RGB -> patch matrices for a list of images that differ in size (lrf_qmf_encode_ragged_rgb_u8;
// host side: lrf_encode8.hip, tables: plan_encode_ragged in lrf_plan.cpp).  The kernels run the bodies of lrf_kernels.hip
// (planes16_unit, planes_strip_unit<KH, KW> — the very functions k_planes16 / k_planes_strip run); what is new is only where a
// workgroup learns its image from: not from blockIdx.y and kernel arguments, but from a table, as in lrf_decode_ragged_kernel.hip.
//
//   blocks[i]      -> (image, unit): which image this workgroup works on and which (strip, column group) inside it
//   descs[image]   -> the image's geometry, size, the offset of its bytes in rgb and of its matrices in the X workspace
//
// Both indices are uniform over the workgroup (blockIdx.x, then a value loaded through it) and both tables are read-only kernel
// arguments, so the entry and the descriptor come in by scalar loads into SGPRs — where the uniform kernels' arguments live — and
// the per-lane code of the bodies is what it is in the uniform kernels.

// all images with sides that are multiples of 16 and 8-byte aligned bytes, in one launch.  grid: the launch's table entries
__global__ __launch_bounds__(256) void k_planes16_ragged(const uint8_t* __restrict__ rgb, float* __restrict__ X, const EncRaggedDesc* __restrict__ descs,
                                                         const RaggedBlock* __restrict__ blocks)
{
    __shared__ __attribute__((aligned(16))) float Ls[2 * 32 * 64];
    const RaggedBlock b = blocks[blockIdx.x];
    const EncRaggedDesc& d = descs[b.image];
    planes16_unit(rgb + d.rgb_off, X + d.x_off, d.H, d.W, d.g, b.tile, Ls);
}

// the other images, one launch per window size (KH, KW) = 2 or 3 by the parity of H and W.  The grid is 8 * xcd_chunk workgroups:
// workgroup i runs on XCD i mod 8, and XCD j takes the contiguous entries [j chunk, (j + 1) chunk) of the launch's table — the
// strips of an image stand together there, so they stay on one XCD (whose L2 then holds the halo rows neighbouring strips share)
// except for the one image per XCD boundary that straddles it.
template <int KH, int KW>
__global__ __launch_bounds__(256) void k_planes_strip_ragged(const uint8_t* __restrict__ rgb, float* __restrict__ X,
                                                             const EncRaggedDesc* __restrict__ descs, const RaggedBlock* __restrict__ blocks, int nblk,
                                                             int xcd_chunk)
{
    __shared__ __attribute__((aligned(16))) float Ls[2 * 32 * 64];
    const int bid = (int)(blockIdx.x & 7) * xcd_chunk + (int)(blockIdx.x >> 3);
    if (bid >= nblk) return;
    const RaggedBlock b = blocks[bid];
    const EncRaggedDesc& d = descs[b.image];
    planes_strip_unit<KH, KW>(rgb + d.rgb_off, X + d.x_off, d.H, d.W, d.g, b.tile, d.per_strip, Ls);
}
