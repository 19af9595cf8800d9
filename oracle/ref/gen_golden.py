"""Regenerate the golden vectors pinned against the REAL reference.

Test infrastructure only. Builds oracle/_ref/ref_harness from the unmodified
pbrt-v4 sources under /root/reference (oracle/ref/Makefile), runs it and writes
  tests/golden/ref_vectors.json                — golden vectors (uint32 float bits)
  tests/golden/hg_edge_vectors.json            — hg_eval / hg_sample at g = 0.0009, -0.0011, -0.99, 1.5
  acceleratedvolrenderer_amd/data/spectra_f32.bin — CIE 1931 x̄ȳz̄, D65 (471 each,
      360..830 nm), sRGB RGBFromXYZ (9), D65 photometric scale, CIE_Y_integral
  tests/golden/camera_ray_vectors.json         — the reference's camera rays of tests/camera_cases.py's cameras
  tests/golden/gaussian_filter_vectors.json    — GaussianFilter::Sample at that module's radii and sigmas
  tests/golden/light_vectors.json              — the reference's light stage at tests/light_cases.py's maps,
      transforms, probes, alias weights, spectra and distant lights
  tests/golden/rgbgrid_vectors.json            — SampledGrid<RGBUnboundedSpectrum / RGBIlluminantSpectrum>::
      Lookup(p, convert) and MaxValue(bounds, convert) over tests/rgbgrid_cases.py's colour grids
The RGB -> spectrum goldens read the sRGB table that the reference's own rgb2spec_opt
writes into oracle/_ref (Makefile); the table stays there (not committed).
The spectral tables are published CIE / ITU data as the reference holds them;
they are inputs to the film, not code.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def main():
    if not os.path.isdir("/root/reference/src/pbrt"):
        sys.exit("reference sources not present; golden vectors are committed")
    subprocess.check_call(["make", "-s", "-j8"], cwd=HERE)
    exe = os.path.join(REPO, "oracle", "_ref", "ref_harness")
    tables = os.path.join(REPO, "acceleratedvolrenderer_amd", "data", "spectra_f32.bin")
    rgbtable = os.path.join(REPO, "oracle", "_ref", "srgb_table.inc")
    out = subprocess.check_output([exe, "--tables", tables, "--rgbtable", rgbtable])
    with open(os.path.join(REPO, "tests", "golden", "ref_vectors.json"), "wb") as f:
        f.write(out)
    edges = subprocess.check_output([exe, "--hg-edges"])
    with open(os.path.join(REPO, "tests", "golden", "hg_edge_vectors.json"), "wb") as f:
        f.write(edges)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, REPO)
    import camera_cases
    rays = subprocess.check_output([exe, "--camera-rays"], input=camera_cases.harness_camera_lines().encode())
    with open(os.path.join(REPO, "tests", "golden", "camera_ray_vectors.json"), "wb") as f:
        f.write(rays)
    filters = subprocess.check_output([exe, "--filters"])
    with open(os.path.join(REPO, "tests", "golden", "gaussian_filter_vectors.json"), "wb") as f:
        f.write(filters)
    import light_cases
    lights = subprocess.check_output([exe, "--rgbtable", rgbtable, "--lights"],
                                     input=light_cases.harness_light_lines().encode())
    with open(os.path.join(REPO, "tests", "golden", "light_vectors.json"), "wb") as f:
        f.write(lights)
    import rgbgrid_cases
    rgbgrid = subprocess.check_output([exe, "--rgbtable", rgbtable, "--rgb-grid"],
                                      input=rgbgrid_cases.harness_lines().encode())
    with open(os.path.join(REPO, "tests", "golden", "rgbgrid_vectors.json"), "wb") as f:
        f.write(rgbgrid)
    print("wrote", len(out), "bytes of golden vectors and", os.path.getsize(tables), "bytes of tables")


if __name__ == "__main__":
    main()
