from stardis_amd.radiation_field.radiation_field_solvers.base import continuum_flux, raytrace  # noqa: F401
