"""Parity of the throughput kernel's doubled orbit trip (render_wave_kernel<1, 2|3>, KIFS_FAST_TRIP_X2_ in
kifs_scene.hpp) with the oracle, on the frames where its exactness argument is thinnest.  A parity check: the kernels
run no test per step that could be observed here.

* Tiny start components: an odd height gives the centre row uv.y = 0, and a camera tilted by 2.5e-21 rad keeps p.z
  near 1e-20 along that row, so z^2 is a denormal number and 4 z^2 rounds differently from z^2.  DESIGN section 4
  argues that w_0^2 = 0.01 absorbs it.
* Remainder trips: 13 SDF iterations (two blocks of six and an odd remainder: the A trip plus the register swap) and
  the reference's 100 (sixteen blocks and four: two pairs; the full divide / square root build).
* A scene outside the host's condition (c.y = 0), which stays on the plain trip.

Each batch holds enough views for the one-wave-per-tile kernel (asserted); the rows around the centre are compared."""
import pytest

from helpers import oracle_frame

pytestmark = pytest.mark.gpu

CFG2_C = (-0.2, 0.6, 0.2, 0.2)


@pytest.mark.parametrize("c, sdf_iters", [(CFG2_C, 12), (CFG2_C, 13), (CFG2_C, 100), ((-0.2, 0.0, 0.2, 0.2), 12)],
                         ids=["cfg2_c_12", "cfg2_c_13", "cfg2_c_100", "c_y_zero_12"])
def test_throughput_kernel_equals_the_oracle_on_tiny_start_components(c, sdf_iters, gs, kifs, oracle):
    import torch
    screen = kifs.ScreenData(1920, 1081)
    gui = kifs.GuiData(fractal_group=kifs.FractalGroup.JuliaSet, constant=c, max_iterations=256)
    iters = (sdf_iters, 10, 10)
    gs.update_screen_data(screen)
    gs.update_options(gui)
    gs.set_iters(*iters)
    H = screen.height
    y0, y1 = H // 2 - 4, H // 2 + 5
    views = 32
    cams = [kifs.CameraData(origin_distance=2.6 + 0.01 * k, phi=0.0, theta=2.5e-21) for k in range(views)]
    outs = [torch.zeros((H, screen.width, 4), dtype=torch.uint8, device="cuda:0") for _ in cams]
    stream = torch.cuda.Stream()
    gs.render_batch_async(outs, cams, stream=stream)
    stream.synchronize()
    assert gs.debug_last_group_tiles() == 0, "the launch should take the throughput kernel (one wave per tile)"
    for k in (0, views // 2, views - 1):
        want = oracle_frame(oracle, kifs, screen, cams[k], gui, iters, y0=y0, y1=y1)
        assert (outs[k][y0:y1].cpu().numpy() == want).all(), k
        assert (want[..., 0] != want[0, 0, 0]).any()  # the centre rows do reach the fractal
