"""rays::trace_render_kernel<G, P> (kifs_trace_rays_async), chosen by dispatch_pipeline<2>(group, primitive,
sdf_iters <= 24): each instantiation is claimed by the geometry_cases.PIPELINES name that reaches it in
test_every_pipeline_bit_exact of tests/test_gpu_rays.py.  A table of its own, in the shape of
kernel_forms.EXTENSION_FORMS and converge_forms.CONVERGE_FORMS: the family's name is deliberately one the form-coverage
pattern of tests/test_kernel_form_coverage.py does not match, so that table stays as it is."""
from kernel_forms import _EXTENSION_PIPELINES

RAY_FORMS = {f"void kifs::rays::trace_render_kernel<{g}, {p}>(kifs::rays::Params)": name
             for (g, p), name in _EXTENSION_PIPELINES.items()}
RAY_TESTS = {"test_gpu_rays.py": RAY_FORMS}
