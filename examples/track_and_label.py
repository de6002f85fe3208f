#!/usr/bin/env python3
"""Consecutive frames to JPEG files whose boxes carry an id that stays with the object, with no detection on the host:

  NV12 frames  --PySurfacePreprocessor.RunTensorBatch (letterbox)-->  (F, 3, 640, 640) float16, and the records it was
                                                                      placed with
  the network  -->  a YOLOv8 head (F, 4 + C, K) whose objects MOVE from frame to frame
  the head     --PyDetectionSelector.Run, four launches-->  dets (F * D, 8) in frame pixels
  dets         --PyDetectionTracker.Run, one launch-->  marks (3 * F * D, 8): outline, label background and label text per
                                                        confirmed track, coloured and labelled by the TRACK'S ID; the
                                                        state is two tensors that live across the batches
  marks        --PySurfaceAnnotator.RunBatch(..., atlas=)-->  drawn in place onto the NV12 frames, two launches
  frames       --PySurfaceConverter, PyNvJpegEncoder(backend="hip")-->  one JPEG file per frame

One stream (a file decoded in batches): every batch holds F consecutive frames, and `tracks` and `clock` carry the
objects from one batch to the next.  The labels are a LabelAtlas of "0" .. "99": a box shows the last two digits of its
id.  Nothing between the network and the encoder reads a detection on the host (ids are fetched for the printout).

    python examples/track_and_label.py [output directory]

Runs on synthetic frames and a made-up head; needs Pillow for the label text."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import python_vali as vali  # noqa: E402

import torch  # noqa: E402

C, K, D, T = 5, 8400, 20, 64
OBJECTS = 7


def network(x, first_frame):
    """a stand-in for a detector on consecutive frames: a raw YOLOv8 head (F, 4 + C, K) float16 in which OBJECTS objects
    drift across the network's input, frame `first_frame + i` in row i; every object is seen by a cluster of candidates
    that NMS thins out, jitters by a pixel or two, and is missed altogether in one frame out of seven"""
    n, dev = x.shape[0], x.device
    g = torch.Generator(device=dev).manual_seed(first_frame)
    o = torch.arange(OBJECTS, device=dev, dtype=torch.float32)
    t = torch.arange(first_frame, first_frame + n, device=dev, dtype=torch.float32)[:, None]
    cx = (60 + 75 * o + (3.0 + o) * t * (1 - 2 * (o % 2))) % 600 + 20                  # (F, OBJECTS)
    cy = 200 + 30 * o + 1.5 * t
    which = torch.randint(0, OBJECTS, (n, K), device=dev, generator=g)
    cxcy = torch.stack([cx.gather(1, which), cy.gather(1, which)], 2) + torch.randn((n, K, 2), device=dev, generator=g) * 1.5
    wh = (50 + 6 * o)[which][..., None].expand(-1, -1, 2) + torch.rand((n, K, 2), device=dev, generator=g) * 4
    scores = torch.rand((n, K, C), device=dev, generator=g) * 0.2
    seen = ((t.long() + 3 * torch.arange(OBJECTS, device=dev)) % 7 != 0).gather(1, which)
    hot = (torch.rand((n, K), device=dev, generator=g) < 0.02) & seen
    scores.scatter_add_(2, (which % C)[..., None],
                        torch.where(hot, 0.45 + 0.45 * torch.rand((n, K), device=dev, generator=g),
                                    torch.zeros((n, K), device=dev))[..., None])
    return torch.cat([cxcy, wh, scores], 2).transpose(1, 2).contiguous().half()


def main():
    out_dir = Path(sys.argv[1]) if len(sys.argv) > 1 else None
    gpu_id, per_batch, batches, w, h = 0, 4, 3, 1280, 720
    device = f"cuda:{gpu_id}"
    rng = np.random.default_rng(0)
    up = vali.PyFrameUploader(gpu_id)
    frames = [vali.Surface.Make(vali.PixelFormat.NV12, w, h, gpu_id) for _ in range(per_batch)]
    cc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_709, vali.ColorRange.MPEG)

    # everything is prepared once; the tensors are rewritten in place batch after batch
    pre = vali.PySurfacePreprocessor(gpu_id, div=255.0)
    x = torch.zeros((per_batch, 3, 640, 640), dtype=torch.float16, device=device)
    pred = torch.zeros((per_batch, 4 + C, K), dtype=torch.float16, device=device)
    labels = vali.LabelAtlas(gpu_id, [str(v) for v in range(100)], pad=2)             # rendered and uploaded once
    style = vali.DetectionStyle(thickness=2, label_rects=labels.rects,
                                colours=[vali.pack_colour(40, 255, 80), vali.pack_colour(255, 200, 0),
                                         vali.pack_colour(80, 160, 255), vali.pack_colour(255, 80, 200),
                                         vali.pack_colour(255, 255, 255)])
    dets = torch.zeros((per_batch * D, 8), dtype=torch.int32, device=device)
    tracked = torch.zeros_like(dets)
    assoc = torch.zeros((per_batch * D, 4), dtype=torch.int32, device=device)
    marks = torch.zeros((3 * per_batch * D, 8), dtype=torch.int32, device=device)
    tracks = torch.zeros((T, 16), dtype=torch.int32, device=device)                   # THE STATE: all zero, no tracks
    clock = torch.zeros((1, 4), dtype=torch.int32, device=device)
    torch.cuda.synchronize()
    tb = pre.PrepareTensorBatch(frames, x, None, [vali.letterbox_rect(w, h, 640, 640)] * per_batch)
    sel = vali.PyDetectionSelector(gpu_id)
    sb = sel.Prepare(pred[:, :4].transpose(1, 2), pred[:, 4:].transpose(1, 2), dets, box_format="cxcywh",
                     max_candidates=1024, max_det=D)
    tk = vali.PyDetectionTracker(gpu_id)
    kb = tk.Prepare(dets, tracks, clock, tracked, assoc, marks, streams=1, max_det=D, max_tracks=T)
    ann = vali.PySurfaceAnnotator(gpu_id)
    ab = ann.PrepareBatch(frames)
    cvt = vali.PySurfaceConverter(gpu_id)
    enc = vali.PyNvJpegEncoder(gpu_id, backend="hip")
    jcc = vali.ColorspaceConversionContext(vali.ColorSpace.BT_601, vali.ColorRange.JPEG)
    planar = [vali.Surface.Make(vali.PixelFormat.YUV420, w, h, gpu_id) for _ in range(per_batch)]

    ids_seen = set()
    for b in range(batches):
        for f in frames:                                                  # stand-ins for PyDecoder's next frames
            assert up.Run(rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8), f)[0]
        ok, info = pre.RunTensorBatch(tb, pad=(114, 114, 114), cc_ctx=cc)
        assert ok, info
        pred.copy_(network(x, b * per_batch))
        torch.cuda.synchronize()                                          # the producer has finished before another stream reads

        ok, info = sel.Run(sb, tb.rects, score_thr=0.25, iou_thr=0.45)                   # four launches
        assert ok, info
        ok, info = tk.Run(kb, iou_thr=0.3, new_thr=0.5, min_hits=3, max_age=30, momentum=0.5, style=style)   # one
        assert ok, info
        ok, info = ann.RunBatch(ab, marks, atlas=labels.surface)                         # two launches
        assert ok, info
        for src, dst in zip(frames, planar):
            ok, info = cvt.Run(src, dst, jcc)
            assert ok, info
        files, info = enc.Run(enc.Context(90, vali.PixelFormat.YUV420), planar)
        assert info == vali.TaskExecInfo.SUCCESS, info

        rows = tracked.cpu().numpy().reshape(per_batch, D, 8)
        for i, f in enumerate(files):
            ids = sorted(int(r[5]) for r in rows[i] if r[0] >= 0)
            ids_seen.update(ids)
            print(f"frame {b * per_batch + i}: ids {ids}, {f.size} bytes of JPEG")
            if out_dir is not None:
                out_dir.mkdir(parents=True, exist_ok=True)
                (out_dir / f"frame_{b * per_batch + i:03d}.jpg").write_bytes(f.tobytes())
    state = clock.cpu().numpy()[0]
    print(f"{len(ids_seen)} ids shown for {OBJECTS} objects; {int(state[0]) - 1} tracks started in {int(state[1])} frames")


if __name__ == "__main__":
    main()
