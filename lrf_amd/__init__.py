"""lrf_amd — MI355X-native QMF image-compression hot path, drop-in for pashtari/lrf's
`lrf.qmf_encode` / `lrf.qmf_decode` / `lrf.QMF`."""
import os as _os

# The pipelined encoder (lrf_pipe) keeps an upload stream and two kernel streams busy next to the caller's own streams.
# The HIP runtime maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and streams that share a queue
# serialise: measured on MI355X, 256 x 512x768 host->host takes 8.7 ms with 4 queues and 6.4 ms with 8.  The variable is
# read when the runtime initialises, so this only helps if lrf_amd is imported before the first GPU call; a value the
# user has set is left alone.
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

from .codec import (ResidentFactors, container_bytes, container_bytes_two_factor, qmf_stream_sizes_gray_ragged, gray_streams_from_device_factors, qmf_decode, qmf_decode_batch, qmf_decode_crops, qmf_decode_ragged, qmf_decode_resized_crops, qmf_decode_scaled, qmf_load_factors, qmf_encode, qmf_encode_batch, qmf_encode_ragged, qmf_encode_sweep, qmf_encode_target, qmf_encode_budget, qmf_stream_sizes, qmf_stream_sizes_ragged, select_budget, select_target_ssim,
                    qmf_factorize_batch, qmf_factorize_host, qmf_ranks)
from .container import (bytes_to_dict, combine_bytes, decode_matrix, decode_tensor, dict_to_bytes, encode_matrix,
                        encode_tensor, separate_bytes)
from .factorization import QMF
from .harness import eval_compression, rd_sweep, rd_sweep_batched
from .rd import LOESS, interpolate_records
from .svd_codec import svd_decode, svd_encode
from .metrics import (bits_per_pixel, compression_ratio, image_metrics_batch, image_metrics_ragged, mse, psnr, psnr_batch, ssim, ssim_batch,
                      sweep_sse_batch)

__all__ = ["qmf_encode", "qmf_decode", "qmf_encode_batch", "qmf_encode_sweep", "qmf_encode_target", "qmf_encode_budget", "qmf_stream_sizes", "qmf_stream_sizes_ragged", "select_budget", "select_target_ssim", "container_bytes", "container_bytes_two_factor", "qmf_stream_sizes_gray_ragged", "gray_streams_from_device_factors", "qmf_decode_batch", "qmf_decode_ragged", "qmf_decode_crops", "qmf_decode_scaled", "qmf_decode_resized_crops", "qmf_load_factors", "ResidentFactors", "qmf_encode_ragged", "qmf_factorize_batch", "qmf_factorize_host", "qmf_ranks", "svd_encode", "svd_decode",
           "QMF", "eval_compression", "rd_sweep", "rd_sweep_batched", "LOESS", "interpolate_records", "psnr", "ssim", "mse", "image_metrics_batch", "image_metrics_ragged", "psnr_batch", "ssim_batch", "sweep_sse_batch", "bits_per_pixel", "compression_ratio", "combine_bytes", "separate_bytes",
           "dict_to_bytes", "bytes_to_dict", "encode_matrix", "decode_matrix", "encode_tensor", "decode_tensor"]
