"""Child process of tests/test_gpu_kernel_forms.py: renders every launch of one configuration of the form table
(tests/kernel_forms.py) and writes, per launch, the observed debug tuples, the first view of every distinct camera and a
digest of every view to an .npz.  The KIFS_TUNING knobs that force the form come with the environment; they are read once
per process, hence one process per configuration.

    python tests/kernel_forms_child.py CONFIG OUT.npz [MODULE]

MODULE (default kernel_forms) supplies plan, SCENES, options, camera and extensions: tests/test_gpu_option_gates.py passes
option_gates.
"""
import hashlib
import importlib
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE)]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import kifs_raymarching_amd as K  # noqa: E402


def main(config, out_path, module="kernel_forms"):
    F = importlib.import_module(module)
    result = {}
    with K.GraphicState(0) as gs:
        for i, L in enumerate(F.plan(config)):
            w, h = L.size
            gs.update_screen_data(K.ScreenData(w, h))
            gs.set_raw_uniforms(options=F.options(K, L.scene))
            gs.set_iters(*F.SCENES[L.scene].iters)
            gs.set_extensions(**F.extensions(L.scene))
            if L.shuffle:
                gs.debug_set_tile_order(F.shuffled_order(w, h))
            y1 = L.y1 if L.y1 is not None else h
            cams = [F.camera(K, L.scene, c) for c in L.cams]
            n = len(cams)
            # 0x5a everywhere: a pixel no kernel wrote keeps alpha 0x5a, which no encode produces
            outs = torch.full((L.repeats, n, L.rows, w, 4), 0x5A, dtype=torch.uint8, device="cuda:0")
            tuples = []
            stream = torch.cuda.Stream()
            if n == 1:  # a lone frame renders the context's camera
                gs.set_camera(cams[0])
            for r in range(L.repeats):
                if n == 1:
                    gs.render(out=outs[r, 0], y0=L.y0, y1=y1, encode=L.encode)
                else:
                    gs.render_batch_async([outs[r, v] for v in range(n)], cams, stream=stream, y0=L.y0, y1=y1,
                                          encode=L.encode)
                    stream.synchronize()
                tuples.append((gs.debug_last_kernel(), gs.debug_last_group_tiles(), gs.debug_last_bunny_form(),
                               gs.debug_last_round_steps()))
            torch.cuda.synchronize()
            host = outs.cpu().numpy()
            first = {}
            for v, c in enumerate(L.cams):
                first.setdefault(c, v)
            result[f"L{i}_kernels"] = np.array([t[0] for t in tuples])
            result[f"L{i}_shape"] = np.array([t[1:] for t in tuples], dtype=np.int32)  # tiles, bunny form, round steps
            result[f"L{i}_cams"] = np.array(sorted(first), dtype=np.int32)
            result[f"L{i}_views"] = np.stack([host[0, first[c]] for c in sorted(first)])
            result[f"L{i}_digests"] = np.array([[hashlib.sha1(host[r, v].tobytes()).hexdigest() for v in range(n)]
                                                for r in range(L.repeats)])
            print(f"{config}: {L.label}: {tuples[-1]}", flush=True)
    np.savez(out_path, **result)


if __name__ == "__main__":
    main(*sys.argv[1:4])
