#!/usr/bin/env python3
"""A network's output straight to JPEG files, in ONE call:

  a float16 batch in [-1, 1] (what a generator, a super-resolution net or a denoiser hands back)
  -> 4:2:0 JPEG files at quality 90, with pixel = clamp(round(x * 127.5 + 127.5), 0, 255).

No float32 copy, no round / clamp / to(uint8) passes, no permute into packed RGB and no surfaces: the encoder's first
kernel reads the 2-byte element, quantises it in registers and goes on with colour conversion, chroma subsampling and
the FDCT.  The torch chain it replaces is run next to it; the files are the same bytes.

    python examples/tensor_to_jpeg.py [out_dir]

Runs on a synthetic batch."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402
from torch.utils.dlpack import to_dlpack  # noqa: E402


def main():
    gpu_id, batch, w, h = 0, 4, 1280, 720
    dev = f"cuda:{gpu_id}"
    # stands in for the network: smooth colour waves with some noise, float16, a little outside [-1, 1] here and there
    yy, xx = torch.meshgrid(torch.linspace(0, 6.28, h, device=dev), torch.linspace(0, 6.28, w, device=dev), indexing="ij")
    phase = torch.arange(batch * 3, device=dev).view(batch, 3, 1, 1)
    x = (1.05 * torch.sin(xx * (1 + phase % 3) + yy * (1 + phase % 2) + phase) +
         0.02 * torch.randn((batch, 3, h, w), device=dev)).to(torch.float16)
    torch.cuda.synchronize()

    enc = vali.PyNvJpegEncoder(gpu_id, backend="hip")
    ctx = enc.Context(90, vali.RGB, subsampling="420")

    # the tensor as it is
    files, info = enc.RunTensor(ctx, x, scale=127.5, offset=127.5)
    assert info == vali.TaskExecInfo.SUCCESS, info

    # the chain it replaces: four elementwise passes with 4-byte intermediates, a permute, N surfaces
    u8 = (x.float() * 127.5 + 127.5).round().clamp(0, 255).to(torch.uint8)
    u8 = u8.permute(0, 2, 3, 1).contiguous()
    torch.cuda.synchronize()
    surfs = [vali.Surface.from_dlpack(to_dlpack(u8[i].view(h, 3 * w)), vali.RGB) for i in range(batch)]
    chain_files, info = enc.Run(ctx, surfs)
    assert info == vali.TaskExecInfo.SUCCESS, info

    # the same pixels in fewer bytes: Huffman tables built on the GPU from each picture's own symbol counts
    small, info = enc.RunTensor(enc.Context(90, vali.RGB, subsampling="420", optimize=True), x, scale=127.5, offset=127.5)
    assert info == vali.TaskExecInfo.SUCCESS, info

    for i, (a, b, c) in enumerate(zip(files, chain_files, small)):
        print(f"item {i}: {a.size} bytes, {'the same file as' if a.tobytes() == b.tobytes() else 'DIFFERS from'} the chain's; "
              f"{c.size} bytes with optimize=True")
    if len(sys.argv) > 1:
        out = Path(sys.argv[1])
        out.mkdir(parents=True, exist_ok=True)
        for i, f in enumerate(files):
            (out / f"item_{i}.jpg").write_bytes(f.tobytes())
        print("written to", out)


if __name__ == "__main__":
    main()
