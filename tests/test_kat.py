"""Per-function known-answer tests: the REFERENCE's own functions (BSDF2 / BSDF_eval2 / BSDF_pdf for every material and
microfacet distribution, Microfacet_D / G1 / pdf / sample, conductor / dielectric reflectance, sphere and quad light
sampling, HomogeneousMedium_sampleDistance, the Henyey-Greenstein phase function, createCamRay, the primitive tests)
were run on seeded inputs by oracle/ref/kat_harness.cl inside the reference build (tests/golden/make_kat.py); the
fixture tests/golden/kat_functions.npz holds inputs and answers.  Here the product's device functions
(csrc/hip/pt_selftest.h) must give the same bits -- compiled for the host (this file, no GPU) and on the GPU
(tests/test_gpu_parity.py::test_device_functions_match_reference_kat).  End-to-end renders reach rare branches only by
luck; these tables reach them by construction (total internal reflection, the Dirac lobes' eval / pdf, C <= 0 in the
sphere sampler, the quad's back face, grazing microfacet configurations, both camera models)."""
from mirrors import assert_kat_equal, check_env_lookup, kat_tables


def test_fixture_covers_the_functions_of_the_path():
    names = [n for n, *_ in kat_tables()]
    assert len(names) >= 40
    for needle in ("bsdf_sample_diff", "bsdf_sample_cond", "bsdf_sample_diel", "bsdf_sample_coat", "bsdf_sample_roughcond_ggx", "bsdf_sample_roughdiel_beckmann",
                   "bsdf_eval_roughdiel_phong", "microfacet_ggx", "fresnel", "light_sphere", "light_quad", "medium", "phase_hg", "camera_pinhole", "hit_quad"):
        assert any(n.startswith(needle) for n in names), needle


def test_device_functions_on_host_match_reference_kat():
    import emu_api
    for name, fn, params, cases, expect, cols in kat_tables():
        assert_kat_equal(name, emu_api.selftest_fn(fn, params, cases), expect, cols)


def test_env_lookup_follows_the_opencl_sampler_rules_on_host():
    import emu_api
    check_env_lookup(emu_api.selftest_fn)
