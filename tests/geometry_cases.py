"""The scenes of the geometry-output tests: one per pipeline geom::render_kernel is instantiated for -- both Julia
variants (the short divide / square root up to 24 orbit iterations, the ordinary ones from 25), the generalised Julia
set, the six primitives and a primitive id outside the enum."""


class Raw:
    """An options image passed through where the helpers expect GuiData (the unknown primitive id)."""

    def __init__(self, u):
        self.u = u

    def into_buffer_data(self):
        return self.u


PIPELINES = ["julia_24", "julia_25", "genjulia", "sphere", "cylinder", "box", "torus", "sierpinski", "bunny", "unknown_id"]


def cases(K, width, height):
    """name -> (screen, camera, gui, iters)."""
    from kifs_raymarching_amd.configs import JULIA_C
    S, Cam, G = K.ScreenData, K.CameraData, K.GuiData
    FG, PS = K.FractalGroup, K.PrimitiveShape
    near = Cam(origin_distance=3.5, phi=0.6, theta=0.5)
    prim = lambda p: G(primitive_shape=p, fractal_color=(250, 120, 60), background_color=(5, 5, 30))
    unknown = G(background_color=(30, 60, 90)).into_buffer_data()
    unknown.primitive_id = 17
    screen = S(width, height)
    julia = G(max_iterations=128, fractal_group=FG.JuliaSet, constant=JULIA_C, background_color=(12, 0, 40))
    return {
        "julia_24": (screen, Cam(origin_distance=3.0, phi=0.3), julia, (24, 10, 10)),
        "julia_25": (screen, Cam(origin_distance=2.5, phi=0.7, theta=0.4), julia, (25, 10, 10)),
        "genjulia": (screen, Cam(origin_distance=3.0, phi=0.5), G(max_iterations=64, fractal_group=FG.GeneralizedJuliaSet,
                                                                  power=3.5), (8, 4, 10)),
        "sphere": (screen, near, prim(PS.Sphere), (100, 10, 10)),
        "cylinder": (screen, near, prim(PS.Cylinder), (100, 10, 10)),
        "box": (screen, near, prim(PS.Box), (100, 10, 10)),
        "torus": (screen, near, prim(PS.Torus), (100, 10, 10)),
        "sierpinski": (screen, Cam(origin_distance=3.0, phi=1.0, theta=0.3),
                       G(primitive_shape=PS.SierpinskiTetrahedron, background_color=(10, 40, 90)), (100, 10, 10)),
        "bunny": (screen, Cam(origin_distance=2.6, phi=2.1, theta=-0.4), prim(PS.Bunny), (100, 10, 10)),
        "unknown_id": (screen, near, Raw(unknown), (100, 10, 10)),
    }
