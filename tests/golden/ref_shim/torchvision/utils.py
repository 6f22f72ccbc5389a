def make_grid(*args, **kwargs):
    raise NotImplementedError('ref_shim: torchvision is not installed; make_grid is not restated')
