"""Renderer — the reference's inference harness [REF thermo_nerf/render/renderer.py:20-228]: walk a camera path, render every
pose, colour the thermal image with ``magma``, quantise to 8 bits, write JPEG frames and a GIF.

What differs from the reference, and why:

* **One render per pose**, whatever the number of modalities: ``RayRenderEngine`` produces every output in one pass and eval
  rendering is deterministic here (tools/race_probe.py), so the frames equal the reference's modality-outer loop
  [REF :180-187] at a third of the work for three modalities.
* **Frames are finished on the device** (``tn_frame_to_rgb8``: colour map / x255 / uint8, bit-equal to the reference's
  matplotlib and numpy expressions [REF :189-199]; DESIGN.md "Frame finishing"): 3 B per pixel and modality cross to the host
  instead of 4-12 B of fp32, into pinned double buffers on a copy stream of their own, while the next pose renders.
* ``RenderedImageModality.RGB.value`` is ``"img"`` but the model's output key is ``"rgb"`` [REF thermal_nerf_model.py:245-248]:
  taken literally, the reference's ``modality.value not in outputs`` raises for RGB.  Here RGB maps to ``outputs["rgb"]``; the
  file names keep ``.value`` (``img_00000.jpeg``).
* ``from_pipeline_path`` unpickles a ``config.yml`` of nerfstudio objects, which ``checkpoint.py`` never touches by design:
  ``from_checkpoint`` takes the model config as an argument instead.
* ``depth_color_map``: opt-in nerfstudio ``apply_depth_colormap`` for DEPTH (the reference scales raw depth by 255).
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch
from PIL import Image
from torch import Tensor

from .. import _hip, colormaps
from ..cameras import Cameras
from ..cameras import load_cameras as _load_cameras
from ..rays import RayBundle
from ..rendered_image_modalities import RenderedImageModality

SCALE, LUT, DEPTH = 0, 1, 2  # TN_FRAME_*


def frame_to_rgb8(src: Tensor, mode: int = SCALE, table: Optional[Tensor] = None, acc: Optional[Tensor] = None,
                  near_far: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """``src`` [..., C] device floats (C 1 or 3) -> uint8 [n, 3] on the device through ``tn_frame_to_rgb8``, on the current stream.
    ``table``: uint8 [256,3] (LUT) or float32 [256,3] (DEPTH); ``acc`` [n] / ``near_far`` [2] device floats (DEPTH).
    ``out``: a uint8 tensor or view of 3 n contiguous bytes, at any byte offset of its allocation."""
    s = _hip.require_device_tensor(src, "src")
    c = s.shape[-1]
    n = s.numel() // max(c, 1)
    if out is None:
        out = torch.empty((n, 3), dtype=torch.uint8, device=s.device)
    if out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() != 3 * n:
        raise ValueError("out must be a contiguous uint8 device tensor of 3 bytes per pixel")
    want = {SCALE: None, LUT: torch.uint8, DEPTH: torch.float32}.get(mode, None)
    if want is not None:
        if table is None or table.dtype != want or tuple(table.shape) != (256, 3) or not table.is_cuda or not table.is_contiguous():
            raise ValueError(f"mode {mode} needs a contiguous {want} [256, 3] device table")
    if mode == DEPTH:
        acc = _hip.require_device_tensor(acc, "acc")
        near_far = _hip.require_device_tensor(near_far, "near_far")
        if acc.numel() != n or near_far.numel() != 2:
            raise ValueError("DEPTH needs one accumulation value per pixel and near_far = 2 floats")
    if n == 0:
        return out
    with torch.cuda.device(s.device):
        _hip.check(_hip.load().tn_frame_to_rgb8(s.data_ptr(), n, c, mode, _hip.ptr(table) if want is not None else None,
                                                _hip.ptr(acc) if mode == DEPTH else None,
                                                _hip.ptr(near_far) if mode == DEPTH else None, out.data_ptr(),
                                                _hip.current_stream()), "tn_frame_to_rgb8")
    return out


def output_key(modality: RenderedImageModality) -> str:
    """the model-output key of a modality: ``.value``, except RGB -> "rgb" (module docstring)"""
    return "rgb" if modality == RenderedImageModality.RGB else modality.value


class Renderer:
    """[REF thermo_nerf/render/renderer.py:20-31]"""

    def __init__(self, model) -> None:
        self._rendered_images: Dict[RenderedImageModality, List[np.ndarray]] = {}
        self._model = model
        self._engine = None

    @property
    def model(self):
        return self._model

    @classmethod
    def from_checkpoint(cls, run_dir, config, num_train_data: int, eval_num_rays_per_chunk: Optional[int] = None,
                        device="cuda", scene_box=None) -> "Renderer":
        """Counterpart of ``from_pipeline_path`` [REF :118-142]: a ThermalNerfModel of ``config`` (the training run's
        ThermalNerfModelConfig) and ``num_train_data`` cameras, loaded from the newest ``*.ckpt`` under ``run_dir``, in eval mode on
        ``device``.  ``eval_num_rays_per_chunk``: as in the reference, overrides the config's value [REF :62-63]."""
        import copy

        from .. import SceneBox, ThermalNerfModel
        from ..checkpoint import latest_checkpoint, load_nerfstudio_checkpoint

        config = copy.copy(config)
        if eval_num_rays_per_chunk is not None:
            config.eval_num_rays_per_chunk = int(eval_num_rays_per_chunk)
        model = ThermalNerfModel(config, metadata={RenderedImageModality.THERMAL.value: []},
                                 scene_box=scene_box if scene_box is not None else SceneBox.unit(), num_train_data=num_train_data)
        load_nerfstudio_checkpoint(model, latest_checkpoint(run_dir))
        model.eval()
        return cls(model.to(device))

    @staticmethod
    def load_cameras(load_camera_trajectory, rendered_resolution_scaling_factor: float = 1.0) -> Cameras:
        """[REF :144-158]"""
        return _load_cameras(load_camera_trajectory, rendered_resolution_scaling_factor)

    # ---- rendering -----------------------------------------------------------------------------------------------------------
    def _render_pose(self, cameras: Cameras, rb: RayBundle, out: Optional[Dict[str, Tensor]]):
        """(outputs, gate): every output of a pose's flat ray bundle as [H*W, C] device floats, queued on the current stream (no
        host synchronisation), and the event behind the first proposal launch of the pose — from there to the end of the pose a
        long kernel is always running (None: the generic loop, which exposes no such point)"""
        model = self._model
        if not model._fusable():  # staged fields (MLP widths other than 64): the model's generic per-chunk loop
            h, w = cameras.height, cameras.width
            res = model.get_outputs_for_camera_ray_bundle(RayBundle(origins=rb.origins.view(h, w, 3), directions=rb.directions.view(h, w, 3)))
            return {k: v.reshape(h * w, -1) for k, v in res.items()}, None
        from ..engine import engine_for

        eng = self._engine = engine_for(model, self._engine)
        eng.timings.clear()
        out = eng.render(rb.origins, rb.directions, out=out, record_events=True)
        gate = eng.timings[0][1] if eng.timings else None
        eng.timings.clear()
        return out, gate

    @torch.no_grad()
    def render(self, rendered_image_modalities: Sequence[RenderedImageModality], cameras: Cameras,
               thermal_color_map: str = "magma", depth_color_map: Optional[str] = None) -> None:
        """[REF :160-201] fills ``self._rendered_images[modality]`` with one uint8 [H, W, 3] numpy array per pose.

        THERMAL: ``thermal_color_map`` lookup (a name of ``colormaps.NAMES``); RGB, ACCUMULATION: x 255; DEPTH: x 255 like the
        reference, or nerfstudio's depth colouring with ``depth_color_map`` (e.g. "turbo").  A modality the model's outputs do not
        hold raises, with the reference's message.

        Timeline of pose k (slot s = k % 2): the current stream (the engine's two streams fork from it and join it) and a copy stream
            current stream   wait copied[s] of pose k-2 | proposal + field kernels of pose k | rays of pose k+1 |
                             finish kernels -> dst[s] | event finished[s]
            copy stream      wait finished[s] and the first proposal launch of pose k+1 | dst[s] -> pinned[s] (non_blocking) |
                             event copied[s]
            host             queue pose k and the copy of pose k-1, then wait copied[1-s] and append the frames of pose k-1 —
                             while pose k renders
        """
        if self._model.training:
            raise RuntimeError("Renderer renders in eval mode; call model.eval() first")
        modalities = list(rendered_image_modalities)
        if self._model._fusable():  # the engine's outputs are known before anything is queued
            from ..engine import OUTPUT_KEYS

            for m in modalities:
                if output_key(m) not in OUTPUT_KEYS:
                    raise Exception(f"{m.value} modality does not exist")  # [REF :189-190]
        dev = torch.device(self._model.device)
        if dev.type != "cuda":
            raise RuntimeError(f"the model is on {dev}; thermo_nerf_amd renders only on a ROCm device (no CPU fallback exists)")
        self._rendered_images = {m: [] for m in modalities}
        h, w = cameras.height, cameras.width
        n, m_count = h * w, len(modalities)
        if m_count == 0 or cameras.size == 0:
            return
        magma_u8 = colormaps.get_table(thermal_color_map, dev)[1]
        depth_f32 = colormaps.get_table(depth_color_map, dev)[0] if depth_color_map else None
        with torch.cuda.device(dev):
            main = torch.cuda.current_stream(dev)
            copy_stream = torch.cuda.Stream(device=dev)
            dst = [torch.empty((m_count, n, 3), dtype=torch.uint8, device=dev) for _ in range(2)]
            pinned = [torch.empty((m_count, n, 3), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            finished = [torch.cuda.Event() for _ in range(2)]
            copied: List[Optional[torch.cuda.Event]] = [None, None]
            near_far = torch.empty(2, dtype=torch.float32, device=dev) if depth_f32 is not None else None
            out = None

            def collect(slot: int) -> None:
                copied[slot].synchronize()
                frames = pinned[slot].numpy()
                for j, m in enumerate(modalities):
                    self._rendered_images[m].append(frames[j].reshape(h, w, 3).copy())

            def queue_copy(slot: int, gate) -> None:
                copy_stream.wait_event(finished[slot])
                if gate is not None:
                    copy_stream.wait_event(gate)
                with torch.cuda.stream(copy_stream):
                    pinned[slot].copy_(dst[slot], non_blocking=True)
                    copied[slot] = torch.cuda.Event()
                    copied[slot].record(copy_stream)

            rays = cameras.generate_rays(0, device=dev, flat=True)
            for k in range(cameras.size):
                s = k % 2
                if copied[s] is not None:
                    main.wait_event(copied[s])  # dst[s] is free once pose k-2 has left it
                out, gate = self._render_pose(cameras, rays, out)
                # the copy of pose k-1 starts once pose k's first proposal launch is through: the copy is a shader blit (0.22 ms per
                # 12 MB), and a kernel that STARTS beside it waits for its end — between two poses that wait is idle time, inside a
                # pose the other stream's kernel keeps the chip busy
                if k > 0:
                    queue_copy(1 - s, gate)
                rays = cameras.generate_rays(k + 1, device=dev, flat=True) if k + 1 < cameras.size else None
                for j, m in enumerate(modalities):
                    key = output_key(m)
                    if key not in out:
                        raise Exception(f"{m.value} modality does not exist")  # [REF :189-190]
                    if m == RenderedImageModality.THERMAL:
                        frame_to_rgb8(out[key], LUT, table=magma_u8, out=dst[s][j])
                    elif m == RenderedImageModality.DEPTH and depth_f32 is not None:
                        lo, hi = torch.aminmax(out[key])
                        torch.stack((lo, hi), out=near_far)
                        frame_to_rgb8(out[key], DEPTH, table=depth_f32, acc=out["accumulation"], near_far=near_far, out=dst[s][j])
                    else:
                        frame_to_rgb8(out[key], SCALE, out=dst[s][j])
                finished[s].record(main)
                if k > 0:
                    collect(1 - s)
            last = (cameras.size - 1) % 2
            queue_copy(last, None)
            collect(last)
            main.wait_stream(copy_stream)

    # ---- writing -------------------------------------------------------------------------------------------------------------
    def save_images(self, modalities: Sequence[RenderedImageModality], output_dir: Union[str, Path]) -> None:
        """[REF :203-214] ``{modality.value}_{idx:05d}.jpeg`` per rendered frame"""
        output_dir = Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        for modality in modalities:
            for idx, image in enumerate(self._rendered_images[modality]):
                Image.fromarray(_displayable(image)).save(output_dir / f"{modality.value}_{idx:05d}.jpeg")

    def save_gif(self, modalities: Sequence[RenderedImageModality], seconds: float, output_dir: Union[str, Path]) -> None:
        """[REF :216-228] ``synthesized_video_{modality.value}.gif``; ``seconds`` is the duration of ONE frame, as the reference
        hands it to imageio.mimsave(duration=...).  Written with PIL, which folds identical consecutive frames into one frame
        of the summed duration."""
        output_dir = Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        for modality in modalities:
            frames = [Image.fromarray(_displayable(image)) for image in self._rendered_images[modality]]
            if not frames:
                raise ValueError(f"no rendered {modality.value} frames to write")
            frames[0].save(output_dir / f"synthesized_video_{modality.value}.gif", save_all=True, append_images=frames[1:],
                           duration=int(round(float(seconds) * 1000)), loop=0)


def _displayable(image: np.ndarray) -> np.ndarray:
    """uint8 [H,W,3], [H,W,1] or [H,W] -> what PIL.Image.fromarray takes"""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    return image[:, :, 0] if image.ndim == 3 and image.shape[-1] == 1 else image
