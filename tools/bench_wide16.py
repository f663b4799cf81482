"""conv5 + max (wide16_kernel with its key memset and finalize) alone on the queue at the headline shape, device events
around 200 launches, five windows: python tools/bench_wide16.py [B N [taps]]; taps = 1 times the T-Nets' conv3
(wide_split_kernel) the same way.  GEOA3_LIB_PATH selects the build (the phase-cut variants of
tools/build_w16_variants.sh give timings only: their results are wrong by construction)."""
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from geoa3_amd import _lib  # noqa: E402
from geoa3_amd.pointnet import pack_wide_fragments, pack_wide_split, pack_wide_split16  # noqa: E402
from tools.bench_conv import timeit  # noqa: E402


def main():
    lib = _lib.load()
    B, N = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (250, 1024)
    taps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)
    X = torch.randn(B, 128, N, generator=g).relu_().cuda()
    W = torch.randn(1024, taps * 128, generator=g) * 0.05
    Wp = pack_wide_fragments(W, taps).cuda()
    Wh, uns = (pack_wide_split16 if taps == 3 else pack_wide_split)(W)
    Wh = Wh.cuda()
    bias = torch.randn(1024, generator=g).cuda()
    out = torch.empty(B, 1024, device="cuda")
    arg = torch.empty(B, 1024, device="cuda", dtype=torch.int32)
    keys = torch.empty(B, 1024, device="cuda", dtype=torch.int64)

    def run():
        return lib.geoa3_debug_wide_fwd(X.data_ptr(), Wp.data_ptr(), Wh.data_ptr(), uns, bias.data_ptr(), out.data_ptr(),
                                        arg.data_ptr(), keys.data_ptr(), B, N, taps, None, s)
    us = [timeit(run, iters=200, warmup=20) for _ in range(5)]
    torch.cuda.synchronize()
    import hashlib
    h = hashlib.sha256(out.cpu().numpy().tobytes() + arg.cpu().numpy().tobytes()).hexdigest()[:16]
    print("%s B=%d N=%d us/launch %s  min %.1f  out+arg sha %s" % ("wide16" if taps == 3 else "wide_split", B, N,
                                                                   " ".join("%.1f" % u for u in us), min(us), h))


if __name__ == "__main__":
    main()
