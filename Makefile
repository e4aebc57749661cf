# Launch layer (reference: Makefile:39-52).  `make fit` is the target the reference's help text
# promises but never defines; it runs the engine-backed fit loop.
PYTHON ?= python
PKG := implicit-image-compression_amd
KWARGS ?=

.PHONY: build fit decode fit8 fit-split test test-gpu bench clean

## build: compile libsiren_fit.so for gfx950
build:
	$(PYTHON) __graft_entry__.py build

## fit: implicit MLP image fitting, e.g. make fit KWARGS="mlp.hidden_size=256 img.height=1024 img.width=1024"
fit: build
	PYTHONPATH=$(PKG) $(PYTHON) -m implicit_image.fit $(KWARGS)

## decode: render a run directory written by fit to a PPM, e.g. make decode KWARGS="decode.dir=outputs/synthetic/siren_synthetic/default decode.truth=synthetic" (decode.bits=16: 16 bits per sample, P6 with maxval 65535)
decode: build
	PYTHONPATH=$(PKG) $(PYTHON) -m implicit_image.decode $(KWARGS)

## fit8: one fit per GPU over a comma sweep (per-image sharding), e.g. KWARGS="img.seed=0,1,2,3,4,5,6,7"
fit8: build
	PYTHONPATH=$(PKG) $(PYTHON) -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
	  -m implicit_image.fit $(KWARGS)

## fit-split: ONE picture across NPROC ranks by image rows (train.pixel_split; rank 0 writes the run directory),
## e.g. make fit-split NPROC=8 KWARGS="img.height=8192 img.width=8192 mlp.hidden_size=1024 mlp.depth=12"
NPROC ?= 8
fit-split: build
	PYTHONPATH=$(PKG) $(PYTHON) -m torch.distributed.run --nnodes=1 --nproc-per-node $(NPROC) --master-addr 127.0.0.1 \
	  -m implicit_image.fit train.pixel_split=true $(KWARGS)

test:
	$(PYTHON) -m pytest tests -x -q -m "not gpu"
test-gpu:
	$(PYTHON) -m pytest tests -x -q -m gpu
bench:
	$(PYTHON) bench.py
clean:
	$(MAKE) -C $(PKG)/csrc clean
