from ..util.registry import Registry

BackboneRegistry = Registry("Backbone")
for _name in ("gagnet", "ae-ncsnpp"):
    BackboneRegistry.declare_out_of_scope(_name, "only the NCSN++ family (reverse-SDE sampling path, BASELINE.json north_star) and the ConvTasNet denoiser are built on this engine")
