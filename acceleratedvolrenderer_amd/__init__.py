"""acceleratedvolrenderer_amd — MI355X-native volumetric path integrator.

A from-scratch HIP/gfx950 implementation of the hot path of tsvdh/AcceleratedVolRenderer
(a pbrt-v4 fork): pbrt's null-scattering VolPathIntegrator — delta-tracking free-flight
sampling, ratio-tracking transmittance, majorant-grid DDA over GridMedium, wavefront
queues with wave64 ballot compaction, RGBFilm accumulation — behind the C-ABI in
include/avr.h. See DESIGN.md.
"""
from . import spectra, transform
from .scene import (GridMedium, DistantLight, UniformInfiniteLight, ImageInfiniteLight, PointLight, SpotLight, OrthographicCamera, PerspectiveCamera, SphericalCamera, RGBFilm, SpectralFilm, spectral_image, GBufferFilm, gbuffer_image,
                    Scene, film_rgb, HomogeneousMedium, CloudMedium, NanoVDBMedium, RGBGridMedium, BoxFilter, GaussianFilter,
                    IndependentSampler, ZSobolSampler)
from .vdb import NanoVDBGrid
from .rgbspectrum import RGBToSpectrumTable
from .integrator import VolPathIntegrator, shard_samples, INTEGRATOR_NAMES
from . import capi
from . import scenes
from . import graph
from . import graph_io
from .capi import GraphIndex, GraphUniform
from .graph import GraphIntegrator, IntegrationAnalyzer

__all__ = ["spectra", "transform", "GridMedium", "DistantLight", "UniformInfiniteLight", "OrthographicCamera",
           "PerspectiveCamera", "SphericalCamera", "RGBFilm", "Scene", "film_rgb", "VolPathIntegrator", "shard_samples",
           "INTEGRATOR_NAMES", "capi", "scenes", "HomogeneousMedium", "CloudMedium", "NanoVDBMedium", "NanoVDBGrid", "RGBGridMedium", "RGBToSpectrumTable",
           "SpectralFilm", "spectral_image", "GBufferFilm", "gbuffer_image", "ImageInfiniteLight", "PointLight", "SpotLight", "BoxFilter", "GaussianFilter", "IndependentSampler", "ZSobolSampler",
           "graph", "graph_io", "GraphIndex", "GraphUniform", "GraphIntegrator", "IntegrationAnalyzer"]
