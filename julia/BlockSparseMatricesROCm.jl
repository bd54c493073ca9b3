# BlockSparseMatricesROCm.jl -- reference-side binding of libbsmrocm.so (include/bsm_rocm.h).
#
# EXPERIMENTAL / NOT EXECUTED IN THIS REPOSITORY: no Julia toolchain exists in the build image, so
# this file has never run.  It is the binding a maintainer of BlockSparseMatrices.jl would add (e.g.
# as a package extension): a matrix opts into the MI355X path through the EXISTING `scheduler=`
# keyword, so no reference signature changes.  The Python mirror
# (blocksparsematrices.jl_amd/matrices.py, entries.py, solvers.py) exercises exactly the same C entry points with the same
# argument conventions and is what the parity tests run.
module BlockSparseMatricesROCm

using LinearAlgebra, LinearMaps
using BlockSparseMatrices
import BlockSparseMatrices: AbstractBlockMatrix, BlockSparseMatrix, SymmetricBlockMatrix,
    VariableBlockCompressedRowStorage

const libbsm = get(ENV, "BSM_ROCM_LIB", "libbsmrocm.so")

# ---- the opt-in scheduler ---------------------------------------------------------------------------
"""
    ROCmScheduler(; device=-1, devices=Int32[], accumulate=0, transpose_image=2, storage=nothing)

`BlockSparseMatrix(...; scheduler=ROCmScheduler())` etc.  `devices = [0, 1, ...]` spreads ONE matrix
over several GPUs of the node (bsm_ctx_t: block rows partitioned by stored bytes, halo exchange over
xGMI) -- the counterpart of the reference's `@tasks` fan-out (src/vbcrs.jl:275-276).
`storage = Float32` stores the values of a Float64 / ComplexF64 matrix in single precision (ComplexF32 for complex
blocks; BSM_F64_F32 / BSM_C128_C64) while x, y and every sum stay in double precision: half the bytes per product.
Single-device only; the values are rounded once, when the handle is created.
"""
struct ROCmScheduler
    device::Int32            # HIP ordinal, -1 = current device
    devices::Vector{Int32}   # non-empty: multi-GPU handle over these ordinals
    accumulate::Int32        # 0 auto, 1 atomics, 2 coloured launches, 3 gather, 4 direct (2-4: bitwise reproducible)
    transpose_image::Int32   # 1: keep a second, transposed ordering for A' / transpose(A); 2: when it is cheap
    storage::Union{Nothing,DataType}  # Float32: mixed precision (values stored in single precision)
end
ROCmScheduler(; device=-1, devices=Int32[], accumulate=0, transpose_image=2, storage=nothing) =
    ROCmScheduler(Int32(device), Int32.(collect(devices)), Int32(accumulate), Int32(transpose_image), storage)
BlockSparseMatrices.isserial(::ROCmScheduler) = true   # no host colouring needed for the GPU path

mutable struct BsmOptions           # mirrors bsm_options (72 bytes)
    struct_size::Int32; device::Int32; scheduler::Int32; accumulate::Int32
    validate::Int32; transpose_image::Int32; own_lo::Int64; own_hi::Int64
    ctx::Ptr{Cvoid}; blocks_memspace::Int64; coloring::Int64
    reserved::NTuple{1,Int64}
end

function _check(rc)
    rc == 0 || error("libbsmrocm: " * unsafe_string(ccall((:bsm_last_error, libbsm), Cstring, ())))
    return nothing
end

const _DTYPE = Dict(Float32 => 0, Float64 => 1, ComplexF32 => 2, ComplexF64 => 3)
# mixed precision: (block / vector type, storage=) -> BSM_F64_F32, BSM_C128_C64
function _dtype(::Type{T}, s::ROCmScheduler) where {T}
    s.storage === nothing && return _DTYPE[T]
    s.storage === Float32 || throw(ArgumentError("storage = $(s.storage): only Float32 (single-precision values)"))
    isempty(s.devices) || throw(ArgumentError("storage = Float32 is single-device only (devices = $(s.devices))"))
    T === Float64 && return 4
    T === ComplexF64 && return 5
    throw(ArgumentError("storage = Float32 needs Float64 or ComplexF64 blocks, not $T"))
end
const ROCmEltype = Union{Float32,Float64,ComplexF32,ComplexF64}

mutable struct Handle
    ptr::Ptr{Cvoid}
    function Handle(p)
        h = new(p)
        finalizer(x -> ccall((:bsm_destroy, libbsm), Cint, (Ptr{Cvoid},), x.ptr), h)
    end
end

# contexts of devices live as long as the process (handles keep a pointer into them)
const _ctxs = Dict{Vector{Int32},Ptr{Cvoid}}()
const _lock = ReentrantLock()
function _ctx(devices::Vector{Int32})
    lock(_lock) do
        get!(_ctxs, devices) do
            out = Ref{Ptr{Cvoid}}(C_NULL)
            _check(ccall((:bsm_ctx_create, libbsm), Cint, (Ptr{Int32}, Int32, Ref{Ptr{Cvoid}}),
                         devices, length(devices), out))
            out[]
        end
    end
end

function _options(s::ROCmScheduler)
    o = Ref(BsmOptions(0, 0, 0, 0, 0, 0, 0, 0, C_NULL, 0, 0, (0,)))
    ccall((:bsm_options_default, libbsm), Cvoid, (Ref{BsmOptions},), o)
    o[].device = s.device
    o[].accumulate = s.accumulate
    o[].transpose_image = isempty(s.devices) ? s.transpose_image : Int32(0)
    isempty(s.devices) || (o[].ctx = _ctx(s.devices))
    return o
end

# ---- handle cache -------------------------------------------------------------------------------------
# The reference's three matrix types are IMMUTABLE structs: they cannot be keys of a WeakKeyDict
# (Julia refuses to attach a finalizer to them).  Every constructor allocates at least one fresh
# mutable Vector per instance (rowptr / colors / diagonalcolors): that vector is the key, so the
# handle dies with the matrix and two matrices never share one.
const _handles = WeakKeyDict{Any,Handle}()
_key(A::VariableBlockCompressedRowStorage) = A.rowptr
_key(A::BlockSparseMatrix) = A.colors
_key(A::SymmetricBlockMatrix) = A.diagonalcolors
handle(A) = lock(() -> get!(() -> _create(A), _handles, _key(A)), _lock)

_ld(b) = Int64(max(stride(b, 2), size(b, 1), 1))   # leading dimension; >= 1 also for 0-row blocks

# A block the C ABI can take: element type T, column-major with unit row stride.  The reference admits any
# AbstractMatrix as a block and counts it as prod(size) (_nnz, src/abstractblockmatrix.jl:65-71): sparse blocks,
# adjoints, views with a row stride are densified ONCE here, at handle creation.
_cblock(::Type{T}, b::StridedMatrix{T}) where {T} = stride(b, 1) == 1 ? b : Matrix{T}(b)
_cblock(::Type{T}, b::AbstractMatrix) where {T} = Matrix{T}(b)
_cblocks(::Type{T}, bs) where {T} = [_cblock(T, b) for b in bs]

# replaces the analysis done by the constructor src/vbcrs.jl:78-122 + the loop :266-288
function _create(A::VariableBlockCompressedRowStorage{T}) where {T}
    nb = length(A.blocks)
    m = Int64[size(b, 1) for b in A.blocks]; n = Int64[size(b, 2) for b in A.blocks]
    rowstart = Int64[A.rowindices[searchsortedlast(A.rowptr, i)] for i in 1:nb]
    colstart = Int64.(A.colindices)
    bl = _cblocks(T, A.blocks)
    ptrs = Ptr{Cvoid}[pointer(b) for b in bl]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve A bl _check(ccall((:bsm_vbcrs_create, libbsm), Cint,
        (Cint, Int64, Int64, Int64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
         Ptr{Int64}, Ptr{Int64}, Ref{BsmOptions}, Ref{Ptr{Cvoid}}),
        _dtype(T, A.scheduler), size(A, 1), size(A, 2), nb, ptrs, m, n, _ld.(bl), rowstart, colstart,
        _options(A.scheduler), out))
    return Handle(out[])
end

# replaces src/blockmatrix.jl:62-109 (+ :225-247)
function _create(A::BlockSparseMatrix{T}) where {T}
    nb = length(A.blocks)
    m = Int64[size(b, 1) for b in A.blocks]; n = Int64[size(b, 2) for b in A.blocks]
    ri = [Vector{Int64}(r) for r in A.rowindices]; ci = [Vector{Int64}(c) for c in A.colindices]
    bl = _cblocks(T, A.blocks)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve A bl ri ci _check(ccall((:bsm_blocksparse_create, libbsm), Cint,
        (Cint, Int64, Int64, Int64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
         Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ref{BsmOptions}, Ref{Ptr{Cvoid}}),
        _dtype(T, A.scheduler), size(A, 1), size(A, 2), nb, Ptr{Cvoid}[pointer(b) for b in bl], m, n,
        _ld.(bl), pointer.(ri), pointer.(ci), _options(A.scheduler), out))
    return Handle(out[])
end

# replaces src/symmetricblockmatrix.jl:73-126 (+ :386-435)
function _create(A::SymmetricBlockMatrix{T}) where {T}
    ds = Int64[size(b, 1) for b in A.diagonals]
    m = Int64[size(b, 1) for b in A.offdiagonals]; n = Int64[size(b, 2) for b in A.offdiagonals]
    di = [Vector{Int64}(d) for d in A.diagonalindices]
    ri = [Vector{Int64}(r) for r in A.rowindices]; ci = [Vector{Int64}(c) for c in A.colindices]
    dg = _cblocks(T, A.diagonals); og = _cblocks(T, A.offdiagonals)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve A dg og di ri ci _check(ccall((:bsm_symmetric_create, libbsm), Cint,
        (Cint, Int64, Int64, Int64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Int64}},
         Int64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Int64}},
         Ptr{Ptr{Int64}}, Ref{BsmOptions}, Ref{Ptr{Cvoid}}),
        _dtype(T, A.scheduler), size(A, 1), size(A, 2), length(ds), Ptr{Cvoid}[pointer(b) for b in dg],
        ds, _ld.(dg), pointer.(di), length(m), Ptr{Cvoid}[pointer(b) for b in og],
        m, n, _ld.(og), pointer.(ri), pointer.(ci), _options(A.scheduler), out))
    return Handle(out[])
end

const ROCmMat = Union{BlockSparseMatrix{<:Any,<:Any,<:Any,ROCmScheduler},
    SymmetricBlockMatrix{<:Any,<:Any,<:Any,<:Any,ROCmScheduler},
    VariableBlockCompressedRowStorage{<:Any,<:Any,<:Any,ROCmScheduler}}
const ROCmOp{Z} = Union{Z,LinearMaps.AdjointMap{<:Any,Z},LinearMaps.TransposeMap{<:Any,Z}}

_op(::ROCmMat) = 0
_op(::LinearMaps.TransposeMap) = 1
_op(::LinearMaps.AdjointMap) = 2
_base(A::ROCmMat) = A
_base(A) = A.lmap

# ---- the drop-in ----------------------------------------------------------------------------------------
# Same signature as src/blockmatrix.jl:225, src/symmetricblockmatrix.jl:386, src/vbcrs.jl:266,343.
# beta === false is Julia's strong zero (src/abstractblockmatrix.jl:27-34).
function _mul!(y, A, x, α::T, β::T, strong::Bool, memspace::Integer, stream::Ptr{Cvoid}, ::Type{T}) where {T}
    h = handle(_base(A))
    a = Ref(α); b = Ref(β)
    GC.@preserve x y _check(ccall((:bsm_mul, libbsm), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ref{T}, Ref{T}, Cint, Cint, Ptr{Cvoid}),
        h.ptr, _op(A), pointer(x), pointer(y), a, b, strong, memspace, stream))
    return y
end

_fits(::Type{T}, s::Number) where {T} = s isa Bool || s isa T || (T <: Complex) || !(s isa Complex)

# fast path: plain host vectors of the matrix' element type (BSM_MEM_HOST; page-lock long-lived
# vectors with `pin!` to make both PCIe copies true DMA)
function LinearMaps._unsafe_mul!(y::Vector{T}, A::ROCmOp{Z}, x::Vector{T}, α::Number, β::Number) where
        {T<:ROCmEltype,Z<:ROCmMat}
    if eltype(_base(A)) === T && _fits(T, α) && _fits(T, β)
        return _mul!(y, A, x, T(α), T(β === false ? 0 : β), β === false, 0, C_NULL, T)
    end
    return _fallback_mul!(y, A, x, α, β)
end

# The 3-argument form.  The reference defines its own for the VBCRS wrappers (src/vbcrs.jl:331-341:
# `fill!(y, zero(T))`, then the 5-argument method with β = true) -- for a ROCmScheduler that would zero y on
# the host, upload it and add: forward Julia's strong zero instead (y never travels to the device).
function LinearMaps._unsafe_mul!(y::AbstractVector, A::ROCmOp{Z}, x::AbstractVector) where {Z<:ROCmMat}
    return LinearMaps._unsafe_mul!(y, A, x, true, false)
end

# everything else LinearMaps may hand over -- SubArray columns of `A * X`, strided views, other
# element types, complex α / β on a real matrix: by linearity through contiguous Vector{T} temporaries.
# NEVER the reference's own loop: its `@tasks ... @set scheduler = ...` cannot run a ROCmScheduler.
function LinearMaps._unsafe_mul!(y::AbstractVector, A::ROCmOp{Z}, x::AbstractVector, α::Number, β::Number) where
        {Z<:ROCmMat}
    return _fallback_mul!(y, A, x, α, β)
end

# Complex vectors under a real operator (bsm_mul_cvec / bsm_mul_multi_cvec): a Float64 operator times ComplexF64 vectors,
# Float32 times ComplexF32, in ONE pass over the matrix.  Pure single-device handles only: mixed storage and multi-GPU
# handles keep the Re / Im split of _fallback_mul!.
_cvec_ok(A, ::Type{C}) where {C} = (R = eltype(_base(A)); R <: Union{Float32,Float64} && C === Complex{R} &&
    _base(A).scheduler.storage === nothing && isempty(_base(A).scheduler.devices))

function _mul_cvec!(y, A, x, α::C, β::C, strong::Bool, memspace::Integer, stream::Ptr{Cvoid}) where {C<:Complex}
    h = handle(_base(A))
    a = Ref(α); b = Ref(β)
    GC.@preserve x y _check(ccall((:bsm_mul_cvec, libbsm), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ref{C}, Ref{C}, Cint, Cint, Ptr{Cvoid}),
        h.ptr, _op(A), pointer(x), pointer(y), a, b, strong, memspace, stream))
    return y
end

function _mul_multi_cvec!(Y, A, X, α::C, β::C, strong::Bool, memspace::Integer, stream::Ptr{Cvoid}) where {C<:Complex}
    h = handle(_base(A))
    a = Ref(α); b = Ref(β)
    GC.@preserve X Y _check(ccall((:bsm_mul_multi_cvec, libbsm), Cint,
        (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ref{C}, Ref{C}, Cint, Cint, Ptr{Cvoid}),
        h.ptr, _op(A), size(X, 2), pointer(X), max(stride(X, 2), 1), pointer(Y), max(stride(Y, 2), 1), a, b, strong,
        memspace, stream))
    return Y
end

function LinearMaps._unsafe_mul!(y::Vector{C}, A::ROCmOp{Z}, x::Vector{C}, α::Number, β::Number) where
        {R<:Union{Float32,Float64},C<:Complex{R},Z<:ROCmMat}
    if eltype(_base(A)) === C && _fits(C, α) && _fits(C, β)  # a complex operator: bsm_mul
        return _mul!(y, A, x, C(α), C(β === false ? 0 : β), β === false, 0, C_NULL, C)
    end
    _cvec_ok(A, C) || return _fallback_mul!(y, A, x, α, β)
    return _mul_cvec!(y, A, x, C(α), C(β === false ? 0 : β), β === false, 0, C_NULL)
end

function LinearMaps._unsafe_mul!(Y::Matrix{C}, A::ROCmOp{Z}, X::Matrix{C}, α::Number, β::Number) where
        {R<:Union{Float32,Float64},C<:Complex{R},Z<:ROCmMat}
    if !(eltype(_base(A)) === C) && _cvec_ok(A, C)
        return _mul_multi_cvec!(Y, A, X, C(α), C(β === false ? 0 : β), β === false, 0, C_NULL)
    end
    return _mul_multi!(Y, A, X, α, β)
end

function _fallback_mul!(y, A, x, α, β)
    T = eltype(_base(A))
    # (one result temporary per product; `convert` copies x only when it is not already a Vector{T})
    gpu(v) = _mul!(Vector{T}(undef, size(A, 1)), A, convert(Vector{T}, v), one(T), zero(T), true, 0, C_NULL, T)
    t = (T <: Real && eltype(x) <: Complex) ? complex.(gpu(real.(x)), gpu(imag.(x))) : gpu(x)
    if β === false
        y .= α .* t
    else
        y .= α .* t .+ β .* y
    end
    return y
end

# `A * X` / mul!(Y, A, X, α, β) with matrices: LinearMaps would loop the columns through the vector
# method (one sweep of A per column); bsm_mul_multi streams A once per 8 columns.
LinearMaps._unsafe_mul!(Y::Matrix{T}, A::ROCmOp{Z}, X::Matrix{T}, α::Number, β::Number) where
    {T<:Union{Float32,Float64},Z<:ROCmMat} = _mul_multi!(Y, A, X, α, β)

function _mul_multi!(Y::Matrix{T}, A, X::Matrix{T}, α::Number, β::Number) where {T}
    if !(eltype(_base(A)) === T && _fits(T, α) && _fits(T, β))
        for k in axes(X, 2)
            _fallback_mul!(view(Y, :, k), A, view(X, :, k), α, β)
        end
        return Y
    end
    h = handle(_base(A))
    a = Ref(T(α)); b = Ref(T(β === false ? 0 : β))
    GC.@preserve X Y _check(ccall((:bsm_mul_multi, libbsm), Cint,
        (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ref{T}, Ref{T}, Cint, Cint, Ptr{Cvoid}),
        h.ptr, _op(A), size(X, 2), X, max(stride(X, 2), 1), Y, max(stride(Y, 2), 1), a, b, β === false, 0, C_NULL))
    return Y
end

"Page-lock a long-lived host vector used as x / y (bsm_host_register); undone by its finalizer."
function pin!(v::Vector)
    _check(ccall((:bsm_host_register, libbsm), Cint, (Ptr{Cvoid}, Int64), v, sizeof(v)))
    finalizer(w -> ccall((:bsm_host_unregister, libbsm), Cint, (Ptr{Cvoid},), w), v)
    return v
end

# mirrors bsm_part_info_t (include/bsm_rocm.h)
struct BsmPartInfo
    device::Int32; pad::Int32
    own_lo::Int64; own_hi::Int64; touched_lo::Int64; touched_hi::Int64
    device_bytes::Int64; nblocks::Int64; col_lo::Int64; col_hi::Int64
    reserved::NTuple{2,Int64}
end

"""
    part_ranges(A) -> Vector{(device, rows, cols)}

The parts of a matrix spread over several GPUs (`ROCmScheduler(devices=[...])`): part p lives on `device`, owns the y
entries `rows` and holds the x entries `cols` of a partitioned product (bsm_part_info; 1-based inclusive ranges).
"""
function part_ranges(A)
    h = handle(_base(A))
    n = length(_base(A).scheduler.devices)   # one part per listed device
    out = NamedTuple{(:device, :rows, :cols),Tuple{Int32,UnitRange{Int64},UnitRange{Int64}}}[]
    for p in 0:n-1
        info = Ref(BsmPartInfo(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, (0, 0)))
        _check(ccall((:bsm_part_info, libbsm), Cint, (Ptr{Cvoid}, Int32, Ref{BsmPartInfo}), h.ptr, p, info))
        push!(out, (device=info[].device, rows=info[].own_lo:info[].own_hi, cols=info[].col_lo:info[].col_hi))
    end
    return out
end

# ---- new values for an existing operator (bsm_update_blocks) --------------------------------------------------
# The reference's structs hold the caller's block matrices BY REFERENCE (src/vbcrs.jl:98,114, src/blockmatrix.jl:26-34):
# after `block(A, i) .= B` the next mul! reads the new values.  The cached handle holds a packed copy instead, so an
# in-place edit is invisible to it until
#     refresh!(A; ids=nothing)
# pushes the struct's CURRENT block contents into it: the structure stays (no analysis, no new handle), only values
# move.  ids: 1-based positions in the handle's block order -- A.blocks (VBCRS, BlockSparseMatrix), diagonals then
# offdiagonals (SymmetricBlockMatrix) -- `nothing` = all.  Host blocks: returns when the image holds them.  ROCArray
# blocks: enqueued on the task-local stream, like a device-vector product.
_updblocks(A::VariableBlockCompressedRowStorage) = A.blocks
_updblocks(A::BlockSparseMatrix) = A.blocks
_updblocks(A::SymmetricBlockMatrix) = vcat(A.diagonals, A.offdiagonals)
_memspace(b) = 0                    # host Matrix (device arrays: 1, below)
_updstream(b) = C_NULL

function refresh!(A::ROCmOp{<:ROCmMat}; ids=nothing)
    B = _base(A)
    T = eltype(B)
    h = handle(B)
    allb = _updblocks(B)
    idv = ids === nothing ? collect(Int64, 1:length(allb)) : Int64.(collect(ids))
    isempty(idv) && return A
    sel = allb[idv]
    ms = _memspace(first(sel))
    bl = ms == 0 ? _cblocks(T, sel) : sel
    st = ms == 0 ? C_NULL : _updstream(first(sel))
    GC.@preserve B bl idv _check(ccall((:bsm_update_blocks, libbsm), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Cint, Ptr{Cvoid}),
        h.ptr, length(idv), idv, Ptr{Cvoid}[pointer(b) for b in bl], _ld.(bl), ms, st))
    return A
end

# ---- device-resident vectors (AMDGPU.jl) -----------------------------------------------------------------
# Iterative solvers keep x / y in HBM: BSM_MEM_DEVICE, enqueued on the task-local HIP stream, no
# synchronisation (the product is 10 us for a C2-sized operator against 74-118 us through host vectors).
# Loaded only where AMDGPU.jl is installed.
if Base.find_package("AMDGPU") !== nothing
    @eval begin
        import AMDGPU
        # refresh! of a struct whose blocks are ROCMatrix: BSM_MEM_DEVICE, the task-local stream
        _memspace(::AMDGPU.ROCMatrix) = 1
        _updstream(::AMDGPU.ROCMatrix) = Base.unsafe_convert(Ptr{Cvoid}, AMDGPU.stream().stream)
        function LinearMaps._unsafe_mul!(y::AMDGPU.ROCVector{T}, A::ROCmOp{Z}, x::AMDGPU.ROCVector{T},
                α::Number, β::Number) where {T<:ROCmEltype,Z<:ROCmMat}
            st = Base.unsafe_convert(Ptr{Cvoid}, AMDGPU.stream().stream)
            if T <: Complex && eltype(_base(A)) !== T && _cvec_ok(A, T)  # complex vectors under a real operator
                return _mul_cvec!(y, A, x, T(α), T(β === false ? 0 : β), β === false, 1, st)
            end
            (eltype(_base(A)) === T && _fits(T, α) && _fits(T, β)) ||
                throw(ArgumentError("device vectors must have the matrix' element type (or, for a real matrix, its " *
                                    "complex type); α, β convertible to it"))
            return _mul!(y, A, x, T(α), T(β === false ? 0 : β), β === false, 1, st, T)
        end
        function LinearMaps._unsafe_mul!(Y::AMDGPU.ROCMatrix{T}, A::ROCmOp{Z}, X::AMDGPU.ROCMatrix{T},
                α::Number, β::Number) where {T<:Union{ComplexF32,ComplexF64},Z<:ROCmMat}
            (eltype(_base(A)) !== T && _cvec_ok(A, T)) ||
                throw(ArgumentError("ROCMatrix right-hand sides: complex vectors under a real operator of their precision"))
            st = Base.unsafe_convert(Ptr{Cvoid}, AMDGPU.stream().stream)
            return _mul_multi_cvec!(Y, A, X, T(α), T(β === false ? 0 : β), β === false, 1, st)
        end

        """
            mul_parts!(yparts, A, xparts, α=true, β=false)

        `mul!` for a matrix spread over several GPUs (`ROCmScheduler(devices=[...])`) with x and y PARTITIONED
        like its block rows: `xparts[p]` / `yparts[p]` are `ROCVector`s on device `devices[p]` holding the
        entries of part p's column / row range (`part_ranges(A)`).  Only the halo a part reads beyond its own
        slice and the y segments it produced for rows of another device travel (bsm_mul_parts, xGMI).
        """
        function mul_parts!(yparts::Vector{<:AMDGPU.ROCVector{T}}, A::ROCmOp{Z}, xparts::Vector{<:AMDGPU.ROCVector{T}},
                α::Number=true, β::Number=false) where {T<:ROCmEltype,Z<:ROCmMat}
            h = handle(_base(A))
            # the C side reads one pointer per part and trusts the part lengths: check both here
            pr = part_ranges(A)
            (length(xparts) == length(pr) && length(yparts) == length(pr)) ||
                throw(DimensionMismatch("mul_parts!: \$(length(pr)) parts, got \$(length(xparts)) x parts and \$(length(yparts)) y parts"))
            for (p, r) in enumerate(pr)
                # include/bsm_rocm.h at bsm_mul_parts: op N reads the column range and delivers the row range, op T / C the reverse
                xr, yr = _op(A) == 0 ? (r.cols, r.rows) : (r.rows, r.cols)
                (length(xparts[p]) == length(xr) && length(yparts[p]) == length(yr)) ||
                    throw(DimensionMismatch("mul_parts!: part \$p holds x[\$(xr)] and y[\$(yr)]"))
            end
            xp = Ptr{Cvoid}[Base.unsafe_convert(Ptr{Cvoid}, pointer(v)) for v in xparts]
            yp = Ptr{Cvoid}[Base.unsafe_convert(Ptr{Cvoid}, pointer(v)) for v in yparts]
            a = Ref(T(α)); b = Ref(T(β === false ? 0 : β))
            GC.@preserve xparts yparts _check(ccall((:bsm_mul_parts, libbsm), Cint,
                (Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ref{T}, Ref{T}, Cint, Ptr{Ptr{Cvoid}}),
                h.ptr, _op(A), xp, yp, a, b, β === false, C_NULL))   # NULL streams: every device's default stream
            return yparts
        end
    end
end

# ---- converters (reference src/vbcrs.jl:150-264) -----------------------------------------------------------
"""
    ROCmVBCRS(A::BlockSparseMatrix | A::SymmetricBlockMatrix)

The reference's `VariableBlockCompressedRowStorage(bsm)` / `(sbm)` converters on the GPU.  For a
SymmetricBlockMatrix the reference materialises `transpose.(offdiagonals)` (twice the off-diagonal
storage, src/vbcrs.jl:222-262); here the bookkeeping (`rowptr`, `colindices`, `rowindices` over the
`ndiag + 2 noff` virtual blocks) is identical -- fetched from the library, bit-exact -- but every
off-diagonal block is stored and streamed once (bsm_vbcrs_create_from_symmetric).
"""
struct ROCmVBCRS{T} <: LinearMaps.LinearMap{T}
    handle::Handle
    size::Tuple{Int,Int}
    rowptr::Vector{Int64}
    colindices::Vector{Int64}
    rowindices::Vector{Int64}
    key::Vector{Int}          # fresh per instance (see _key)
end
Base.size(A::ROCmVBCRS) = A.size
_key(A::ROCmVBCRS) = A.key
handle(A::ROCmVBCRS) = A.handle
_base(A::ROCmVBCRS) = A
_op(::ROCmVBCRS) = 0

function _bookkeeping(h::Handle, which::Integer)
    len = Ref{Int64}(0)
    _check(ccall((:bsm_get_bookkeeping, libbsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}, Ref{Int64}), h.ptr, which, C_NULL, len))
    out = Vector{Int64}(undef, len[])
    _check(ccall((:bsm_get_bookkeeping, libbsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}, Ref{Int64}), h.ptr, which, out, len))
    return out
end

# how often products of A have streamed its value image since it was created (bsm_value_passes): a product with K
# columns that adds K ran column by column, one that adds 1 streamed the matrix once
function value_passes(A)
    n = Ref{Int64}(0)
    _check(ccall((:bsm_value_passes, libbsm), Cint, (Ptr{Cvoid}, Ref{Int64}), handle(_base(A)).ptr, n))
    return n[]
end

function ROCmVBCRS(A::SymmetricBlockMatrix{T}; scheduler::ROCmScheduler=ROCmScheduler()) where {T<:ROCmEltype}
    ds = Int64[size(b, 1) for b in A.diagonals]
    m = Int64[size(b, 1) for b in A.offdiagonals]; n = Int64[size(b, 2) for b in A.offdiagonals]
    d0 = Int64[first(d) for d in A.diagonalindices]        # first(...): src/vbcrs.jl:231-239
    r0 = Int64[first(r) for r in A.rowindices]; c0 = Int64[first(c) for c in A.colindices]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve A _check(ccall((:bsm_vbcrs_create_from_symmetric, libbsm), Cint,
        (Cint, Int64, Int64, Int64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
         Int64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
         Ref{BsmOptions}, Ref{Ptr{Cvoid}}),
        _dtype(T, scheduler), size(A, 1), size(A, 2), length(ds), Ptr{Cvoid}[pointer(b) for b in A.diagonals],
        ds, _ld.(A.diagonals), d0, length(m), Ptr{Cvoid}[pointer(b) for b in A.offdiagonals],
        m, n, _ld.(A.offdiagonals), r0, c0, _options(scheduler), out))
    h = Handle(out[])
    return ROCmVBCRS{T}(h, (size(A, 1), size(A, 2)), _bookkeeping(h, 1), _bookkeeping(h, 2), _bookkeeping(h, 3), Int[])
end

function ROCmVBCRS(A::BlockSparseMatrix{T}; scheduler::ROCmScheduler=ROCmScheduler()) where {T<:ROCmEltype}
    nb = length(A.blocks)
    m = Int64[size(b, 1) for b in A.blocks]; n = Int64[size(b, 2) for b in A.blocks]
    ri = [Vector{Int64}(r) for r in A.rowindices]; ci = [Vector{Int64}(c) for c in A.colindices]
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve A ri ci _check(ccall((:bsm_vbcrs_create_from_blocksparse, libbsm), Cint,
        (Cint, Int64, Int64, Int64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64},
         Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ref{BsmOptions}, Ref{Ptr{Cvoid}}),
        _dtype(T, scheduler), size(A, 1), size(A, 2), nb, Ptr{Cvoid}[pointer(b) for b in A.blocks], m, n,
        _ld.(A.blocks), pointer.(ri), pointer.(ci), _options(scheduler), out))
    h = Handle(out[])
    return ROCmVBCRS{T}(h, (size(A, 1), size(A, 2)), _bookkeeping(h, 1), _bookkeeping(h, 2), _bookkeeping(h, 3), Int[])
end

const ROCmViewOp = Union{ROCmVBCRS,LinearMaps.AdjointMap{<:Any,<:ROCmVBCRS},LinearMaps.TransposeMap{<:Any,<:ROCmVBCRS}}
function LinearMaps._unsafe_mul!(y::AbstractVector, A::ROCmViewOp, x::AbstractVector, α::Number, β::Number)
    T = eltype(_base(A))
    if y isa Vector{T} && x isa Vector{T} && _fits(T, α) && _fits(T, β)
        return _mul!(y, A, x, T(α), T(β === false ? 0 : β), β === false, 0, C_NULL, T)
    end
    return _fallback_mul!(y, A, x, α, β)
end
LinearMaps._unsafe_mul!(y::AbstractVector, A::ROCmViewOp, x::AbstractVector) =
    LinearMaps._unsafe_mul!(y, A, x, true, false)

# ---- A[I, J] and diag(A): entries read out of the packed image ---------------------------------------------------
# LinearMaps answers getindex with one product per requested column (unit vectors); bsm_submatrices reads the
# entries in ONE pass over the image, and only the strips that hold a requested column.  Host results, synchronous.
const ROCmAnyOp = Union{ROCmOp{<:ROCmMat},ROCmViewOp}

"""
    submatrices(A, rowsets, colsets=rowsets)

`[A[I, J] for (I, J) in zip(rowsets, colsets)]` in one pass over the image.  The row sets must be pairwise disjoint
and free of repeats, and so must the column sets: `submatrices(S, S.diagonalindices)` gives the block-Jacobi blocks
of a SymmetricBlockMatrix.  Overlapping blocks add, like `sparse(A)`.
"""
function submatrices(A::ROCmAnyOp, rowsets, colsets=rowsets)
    T = eltype(_base(A))
    length(rowsets) == length(colsets) || throw(DimensionMismatch("one column set per row set"))
    I = [collect(Int64, r) for r in rowsets]; J = [collect(Int64, c) for c in colsets]
    outs = [Matrix{T}(undef, length(i), length(j)) for (i, j) in zip(I, J)]
    ni = Int64[length(i) for i in I]; nj = Int64[length(j) for j in J]
    GC.@preserve I J outs _check(ccall((:bsm_submatrices, libbsm), Cint,
        (Ptr{Cvoid}, Cint, Int64, Ptr{Ptr{Int64}}, Ptr{Int64}, Ptr{Ptr{Int64}}, Ptr{Int64}, Ptr{Ptr{Cvoid}}, Ptr{Int64},
         Cint, Ptr{Cvoid}),
        handle(_base(A)).ptr, _op(A), length(I), pointer.(I), ni, pointer.(J), nj,
        Ptr{Cvoid}[pointer(o) for o in outs], max.(ni, 1), 0, C_NULL))
    return outs
end

# repeated indices are extracted once and expanded here (the C entry takes sets)
function _getindex(A::ROCmAnyOp, I::AbstractVector{<:Integer}, J::AbstractVector{<:Integer})
    checkbounds(Bool, 1:size(A, 1), I) && checkbounds(Bool, 1:size(A, 2), J) || throw(BoundsError(A, (I, J)))
    ui = unique(I); uj = unique(J)
    S = submatrices(A, [ui], [uj])[1]
    return S[indexin(I, ui), indexin(J, uj)]
end
const _Idx = Union{Integer,AbstractVector{<:Integer},Colon}
_idx(::Colon, n) = 1:n
_idx(i::Integer, n) = [i]
_idx(v::AbstractVector{Bool}, n) = (length(v) == n || throw(BoundsError(1:n, v)); findall(v))
_idx(v::AbstractVector{<:Integer}, n) = v
function Base.getindex(A::ROCmAnyOp, i::_Idx, j::_Idx)
    S = _getindex(A, _idx(i, size(A, 1)), _idx(j, size(A, 2)))
    i isa Integer && j isa Integer && return S[1, 1]
    i isa Integer && return S[1, :]
    j isa Integer && return S[:, 1]
    return S
end

function LinearAlgebra.diag(A::ROCmAnyOp)
    T = eltype(_base(A))
    d = Vector{T}(undef, min(size(A)...))
    GC.@preserve d _check(ccall((:bsm_diag, libbsm), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}),
        handle(_base(A)).ptr, pointer(d), 0, C_NULL))
    return _op(A) == 2 ? conj!(d) : d
end

# ---- block-Jacobi: the self-interaction blocks inverted in one batched call ---------------------------------------
"""
    invert_blocks!(blocks) -> info

Inverts the square matrices of `blocks` in place (bsm_invert_blocks: Gauss-Jordan elimination with partial row
pivoting, orders 0 .. 1024).  `info[b] == 0`: block `b` holds its inverse; `info[b] == k`: the pivot of step `k` was
zero or not finite and the block is unspecified.  Host matrices run the elimination on the host.
"""
function invert_blocks!(blocks::AbstractVector{Matrix{T}}) where {T<:ROCmEltype}
    all(b -> size(b, 1) == size(b, 2), blocks) || throw(DimensionMismatch("invert_blocks! takes square blocks"))
    n = Int64[size(b, 1) for b in blocks]
    info = zeros(Int64, length(blocks))
    GC.@preserve blocks _check(ccall((:bsm_invert_blocks, libbsm), Cint,
        (Cint, Int64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Cint, Ptr{Cvoid}),
        _DTYPE[T], length(blocks), Ptr{Cvoid}[pointer(b) for b in blocks], n, max.(n, 1), info, 0, C_NULL))
    return info
end

"""
    eigh_blocks!(blocks; vectors=true) -> (w, info)

Eigendecomposition of the square Hermitian matrices of `blocks` in place (bsm_eigh_blocks: two-sided round-robin Jacobi in
the blocks' own type, orders 0 .. 512).  `w[b]` holds the eigenvalues of `(B + B') / 2` ascending, block `b` its orthonormal
eigenvectors as columns (`vectors=false`: unspecified contents).  `info[b]`: 0 done, 1 a non-finite entry (the block is
untouched, `w[b]` is NaN), 2 the cap of 60 sweeps was hit.  Host matrices run the rotations on the host.
"""
function eigh_blocks!(blocks::AbstractVector{Matrix{T}}; vectors::Bool=true) where {T<:ROCmEltype}
    all(b -> size(b, 1) == size(b, 2), blocks) || throw(DimensionMismatch("eigh_blocks! takes square blocks"))
    n = Int64[size(b, 1) for b in blocks]
    w = [Vector{real(T)}(undef, k) for k in n]
    info = zeros(Int64, length(blocks))
    GC.@preserve blocks w _check(ccall((:bsm_eigh_blocks, libbsm), Cint,
        (Cint, Int64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Cvoid}}, Int32, Ptr{Int64}, Ptr{Int32}, Cint, Ptr{Cvoid}),
        _DTYPE[T], length(blocks), Ptr{Cvoid}[pointer(b) for b in blocks], n, max.(n, 1), Ptr{Cvoid}[pointer(x) for x in w],
        vectors ? 1 : 0, info, C_NULL, 0, C_NULL))
    return w, info
end

const _SPEC_FUNC = Dict(:values => 0, :inv => 1, :absinv => 2, :pinv => 3)

"""
    spectral_blocks!(out, V, w; func=:inv, rcond=0.0) -> info

`out[b] = V[b] * Diagonal(f.(w[b])) * V[b]'` (bsm_spectral_blocks), Hermitian to the bit.  `func`: `:values` (f = w), `:inv`
(1 / w), `:absinv` (1 / max(|w|, rcond * max|w|): positive definite) or `:pinv` (1 / w where |w| > rcond * max|w|, else 0).
`info[b]` is 0, or the index of the first eigenvalue at which `f` is undefined (`out[b]` is then not written).
"""
function spectral_blocks!(out::AbstractVector{Matrix{T}}, V::AbstractVector{Matrix{T}}, w::AbstractVector{<:Vector}; func::Symbol=:inv,
                          rcond::Real=0.0) where {T<:ROCmEltype}
    n = Int64[size(b, 1) for b in V]
    all(k -> size(V[k]) == size(out[k]) == (n[k], n[k]) && length(w[k]) == n[k] && eltype(w[k]) == real(T), eachindex(V)) ||
        throw(DimensionMismatch("spectral_blocks! takes square blocks, outputs of their shapes and real eigenvalue vectors"))
    info = zeros(Int64, length(V))
    GC.@preserve out V w _check(ccall((:bsm_spectral_blocks, libbsm), Cint,
        (Cint, Int64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Cvoid}}, Int32, Float64, Ptr{Ptr{Cvoid}}, Ptr{Int64}, Ptr{Int64}, Cint,
         Ptr{Cvoid}),
        _DTYPE[T], length(V), Ptr{Cvoid}[pointer(b) for b in V], n, max.(n, 1), Ptr{Cvoid}[pointer(x) for x in w], _SPEC_FUNC[func],
        Float64(rcond), Ptr{Cvoid}[pointer(b) for b in out], max.(n, 1), info, 0, C_NULL))
    return info
end

"""
    block_jacobi(A, sets=A.diagonalindices; kind=:inverse, rcond=nothing, scheduler=ROCmScheduler())

The block-Jacobi preconditioner `M = sum_s E_s inv(A[I_s, I_s]) E_s'` of a square operator as a `BlockSparseMatrix` on
the MI355X path: `submatrices(A, sets)`, `invert_blocks!`, and the reference's own constructor.  The sets must be
pairwise disjoint and free of repeats; rows in no set are zero rows of `M` (pass singleton sets for point-Jacobi
rows).  Throws `SingularException(s)` for the first set whose block is singular to working precision.

`kind` (with `A[I_s, I_s] = V diag(w) V'`, the blocks taken as Hermitian): `:inverse` as above (`rcond` must be `nothing`);
`:abs` gives `V diag(1 / |w|) V'`, Hermitian positive definite for an indefinite `A` (`rcond`, default 0, clamps `|w|` at
`rcond * max|w|`; a zero eigenvalue throws `SingularException(s)`); `:pinv` the Hermitian pseudo-inverse (`rcond` defaults to
`sqrt(eps)`).  Through `eigh_blocks!` and `spectral_blocks!`.
"""
function block_jacobi(A::ROCmAnyOp, sets=_base(A).diagonalindices; kind::Symbol=:inverse, rcond=nothing,
                      scheduler::ROCmScheduler=ROCmScheduler())
    size(A, 1) == size(A, 2) || throw(DimensionMismatch("block_jacobi needs a square operator"))
    kind in (:inverse, :abs, :pinv) || throw(ArgumentError("kind must be :inverse, :abs or :pinv"))
    I = [collect(Int64, s) for s in sets]
    blocks = submatrices(A, I)
    if kind == :inverse
        rcond === nothing || throw(ArgumentError("rcond has no meaning with kind = :inverse"))
        info = invert_blocks!(blocks)
    else
        rc = rcond === nothing ? (kind == :abs ? 0.0 : sqrt(eps(real(eltype(_base(A)))))) : Float64(rcond)
        w, einfo = eigh_blocks!(blocks)
        s = findfirst(!iszero, einfo)
        s === nothing || throw(ArgumentError("block_jacobi: A[I, I] of set $s is not finite or did not converge"))
        out = [similar(b) for b in blocks]
        info = spectral_blocks!(out, blocks, w; func=(kind == :abs ? :absinv : :pinv), rcond=rc)
        blocks = out
    end
    s = findfirst(!iszero, info)
    s === nothing || throw(LinearAlgebra.SingularException(s))
    return BlockSparseMatrix(blocks, I, I, size(A); scheduler=scheduler)
end

# ---- restarted GMRES on the device (bsm_gmres_*) ----------------------------------------------------------------------
mutable struct BsmGmresParams       # mirrors bsm_gmres_params (40 bytes)
    struct_size::Int32; use_x0::Int32; rtol::Float64; atol::Float64; maxiter::Int64; history_capacity::Int64
end
mutable struct BsmGmresInfo         # mirrors bsm_gmres_info (64 bytes)
    status::Int32; cycles::Int32; iterations::Int64; residual::Float64; bnorm::Float64
    a_products::Int64; m_products::Int64; workspace_bytes::Int64; workspace::UInt64
end

"""
    gmres!(x, A, b; M=nothing, restart=30, rtol=1e-8, atol=0.0, maxiter=size(A, 1), x0=false) -> (x, info, history)

Right-preconditioned restarted GMRES for `A x = b`, every step of it on the device (bsm_gmres_create / _solve /
_destroy): `A` (and the preconditioner `M`, e.g. `block_jacobi(A)`) are matrices on the MI355X path or their
`transpose` / `adjoint` wrappers; `b` and `x` are host vectors of `A`'s element type, or complex ones of its precision
under real `A` and `M`.  Converged when the residual estimate is `<= max(rtol * norm(b), atol)`.  `x0 = true` takes
the incoming `x` as the initial guess.  `info.status`: 0 converged, 1 `maxiter` reached, 2 a non-finite residual;
`history[i]` is the absolute estimate after iteration `i`.  (The reference offers nothing here: a `LinearMap` is
handed to a Julia solver package, whose Krylov loop runs on the host.)
"""
function gmres!(x::Vector{T}, A::ROCmAnyOp, b::Vector{T}; M=nothing, restart::Integer=30, rtol::Real=1e-8, atol::Real=0.0,
                maxiter::Integer=size(A, 1), x0::Bool=false) where {T<:ROCmEltype}
    size(A, 1) == size(A, 2) == length(b) == length(x) || throw(DimensionMismatch("gmres! needs a square operator and vectors of its order"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    mptr = M === nothing ? C_NULL : handle(_base(M)).ptr
    _check(ccall((:bsm_gmres_create, libbsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Int32, Ref{Ptr{Cvoid}}),
        handle(_base(A)).ptr, _op(A), mptr, M === nothing ? 0 : _op(M), _DTYPE[T], restart, out))
    p = BsmGmresParams(sizeof(BsmGmresParams), x0, rtol, atol, maxiter, maxiter)
    info = BsmGmresInfo(0, 0, 0, 0.0, 0.0, 0, 0, 0, 0)
    history = zeros(Float64, max(maxiter, 1))
    try
        GC.@preserve A M x b history _check(ccall((:bsm_gmres_solve, libbsm), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{BsmGmresParams}, Ref{BsmGmresInfo}, Ptr{Float64}, Cint, Ptr{Cvoid}),
            out[], pointer(b), pointer(x), p, info, history, 0, C_NULL))
    finally
        ccall((:bsm_gmres_destroy, libbsm), Cint, (Ptr{Cvoid},), out[])
    end
    return x, info, history[1:min(info.iterations, maxiter)]
end

# ---- CG / COCG on several right-hand sides in lockstep, on the device (bsm_cg_*) -----------------------------------------
mutable struct BsmCgParams          # mirrors bsm_cg_params (40 bytes)
    struct_size::Int32; use_x0::Int32; rtol::Float64; atol::Float64; maxiter::Int64; history_capacity::Int64
end
mutable struct BsmCgInfo            # mirrors bsm_cg_info (48 bytes)
    status::Int32; columns_converged::Int32; iterations::Int64
    a_products::Int64; m_products::Int64; workspace_bytes::Int64; workspace::UInt64
end
mutable struct BsmLsqrParams        # mirrors bsm_lsqr_params (56 bytes)
    struct_size::Int32; use_x0::Int32; rtol::Float64; atol::Float64; ntol::Float64; damp::Float64
    maxiter::Int64; history_capacity::Int64
end
struct BsmCgColumn                  # mirrors bsm_cg_column (32 bytes)
    status::Int32; reserved::Int32; iterations::Int64; residual::Float64; bnorm::Float64
end

"""
    cg!(X, A, B; M=nothing, method=:cg, rtol=1e-8, atol=0.0, maxiter=size(A, 1), x0=false) -> (X, info, columns, history)

Preconditioned conjugate gradients for `A X = B` with 1 to 16 right-hand sides advancing in lockstep on one multi-column
product per iteration, every step of it on the device (bsm_cg_create / _solve / _destroy).  `method = :cg` is for real
symmetric / Hermitian positive definite `A` (and `M`), `method = :cocg` (the unconjugated form) for complex symmetric
ones, e.g. a `SymmetricBlockMatrix` with complex blocks; the caller asserts the symmetry.  `B` and `X` are host vectors
or matrices of `A`'s element type, or complex ones of its precision under real `A` and `M`.  Column `c` is converged when
its residual norm is `<= max(rtol * norm(B[:, c]), atol)`.  `columns[c].status`: 0 converged, 1 `maxiter` reached, 2 a
non-finite residual, 3 breakdown; `history[c, i]` is the residual norm of column `c` after iteration `i`.  (The reference
offers nothing here: a `LinearMap` is handed to a Julia solver package, whose Krylov loop runs on the host.)
"""
function cg!(X::VecOrMat{T}, A::ROCmAnyOp, B::VecOrMat{T}; M=nothing, method::Symbol=:cg, rtol::Real=1e-8, atol::Real=0.0,
             maxiter::Integer=size(A, 1), x0::Bool=false) where {T<:ROCmEltype}
    n, k = size(B, 1), size(B, 2)
    size(A, 1) == size(A, 2) == n && size(X) == size(B) || throw(DimensionMismatch("cg! needs a square operator and B, X of its order"))
    1 <= k <= 16 || throw(ArgumentError("cg! takes 1 to 16 right-hand sides"))
    method in (:cg, :cocg) || throw(ArgumentError("method must be :cg or :cocg"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    mptr = M === nothing ? C_NULL : handle(_base(M)).ptr
    _check(ccall((:bsm_cg_create, libbsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Int32, Int32, Ref{Ptr{Cvoid}}),
        handle(_base(A)).ptr, _op(A), mptr, M === nothing ? 0 : _op(M), _DTYPE[T], k, method === :cg ? 0 : 1, out))
    p = BsmCgParams(sizeof(BsmCgParams), x0, rtol, atol, maxiter, maxiter)
    info = BsmCgInfo(0, 0, 0, 0, 0, 0, 0)
    columns = Vector{BsmCgColumn}(undef, k)
    history = zeros(Float64, k, max(maxiter, 1))
    ld = max(n, 1)
    try
        GC.@preserve A M X B columns history _check(ccall((:bsm_cg_solve, libbsm), Cint,
            (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ref{BsmCgParams}, Ref{BsmCgInfo}, Ptr{BsmCgColumn}, Ptr{Float64}, Cint, Ptr{Cvoid}),
            out[], k, pointer(B), ld, pointer(X), ld, p, info, columns, history, 0, C_NULL))
    finally
        ccall((:bsm_cg_destroy, libbsm), Cint, (Ptr{Cvoid},), out[])
    end
    return X, info, columns, history[:, 1:min(info.iterations, maxiter)]
end

"""
    gmres!(X, A, B; M=nothing, restart=30, rtol=1e-8, atol=0.0, maxiter=size(A, 1), x0=false) -> (X, info, columns, history)

Right-preconditioned restarted GMRES for `A X = B` with 1 to 16 right-hand sides advancing in lockstep on one multi-column
product per iteration, every step of it on the device (bsm_gmres_multi_create / _solve / _destroy).  Per column it is the
method of the vector form of `gmres!`; all columns restart together.  `info`, `columns` and `history` are those of
[`cg!`](@ref), `history` holding the residual estimates: `columns[c].status` 0 converged, 1 `maxiter` reached, 2 a
non-finite residual; the cycles are `cld(info.iterations, restart)`.
"""
function gmres!(X::Matrix{T}, A::ROCmAnyOp, B::Matrix{T}; M=nothing, restart::Integer=30, rtol::Real=1e-8, atol::Real=0.0,
                maxiter::Integer=size(A, 1), x0::Bool=false) where {T<:ROCmEltype}
    n, k = size(B, 1), size(B, 2)
    size(A, 1) == size(A, 2) == n && size(X) == size(B) || throw(DimensionMismatch("gmres! needs a square operator and B, X of its order"))
    1 <= k <= 16 || throw(ArgumentError("gmres! takes 1 to 16 right-hand sides"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    mptr = M === nothing ? C_NULL : handle(_base(M)).ptr
    _check(ccall((:bsm_gmres_multi_create, libbsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Int32, Int32, Ref{Ptr{Cvoid}}),
        handle(_base(A)).ptr, _op(A), mptr, M === nothing ? 0 : _op(M), _DTYPE[T], k, restart, out))
    p = BsmCgParams(sizeof(BsmCgParams), x0, rtol, atol, maxiter, maxiter)
    info = BsmCgInfo(0, 0, 0, 0, 0, 0, 0)
    columns = Vector{BsmCgColumn}(undef, k)
    history = zeros(Float64, k, max(maxiter, 1))
    ld = max(n, 1)
    try
        GC.@preserve A M X B columns history _check(ccall((:bsm_gmres_multi_solve, libbsm), Cint,
            (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ref{BsmCgParams}, Ref{BsmCgInfo}, Ptr{BsmCgColumn}, Ptr{Float64}, Cint, Ptr{Cvoid}),
            out[], k, pointer(B), ld, pointer(X), ld, p, info, columns, history, 0, C_NULL))
    finally
        ccall((:bsm_gmres_multi_destroy, libbsm), Cint, (Ptr{Cvoid},), out[])
    end
    return X, info, columns, history[:, 1:min(info.iterations, maxiter)]
end

"""
    bicgstab!(X, A, B; M=nothing, rtol=1e-8, atol=0.0, maxiter=size(A, 1), x0=false) -> (X, info, columns, history)

Right-preconditioned BiCGSTAB for `A X = B` with `A` not necessarily symmetric and 1 to 16 right-hand sides advancing in
lockstep on two multi-column products per iteration, every step of it on the device (bsm_bicgstab_create / _solve /
_destroy).  `B` and `X` are host vectors or matrices of `A`'s element type, or complex ones of its precision under real
`A` and `M`.  Column `c` is converged when its residual norm, after either half of an iteration, is
`<= max(rtol * norm(B[:, c]), atol)`.  `info`, `columns` and `history` are those of [`cg!`](@ref): `columns[c].status` 0
converged, 1 `maxiter` reached, 2 a non-finite residual, 3 breakdown; `info.a_products == 2 * info.iterations`.  (The
reference offers nothing here: a `LinearMap` is handed to a Julia solver package, whose Krylov loop runs on the host.)
"""
function bicgstab!(X::VecOrMat{T}, A::ROCmAnyOp, B::VecOrMat{T}; M=nothing, rtol::Real=1e-8, atol::Real=0.0,
                   maxiter::Integer=size(A, 1), x0::Bool=false) where {T<:ROCmEltype}
    n, k = size(B, 1), size(B, 2)
    size(A, 1) == size(A, 2) == n && size(X) == size(B) || throw(DimensionMismatch("bicgstab! needs a square operator and B, X of its order"))
    1 <= k <= 16 || throw(ArgumentError("bicgstab! takes 1 to 16 right-hand sides"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    mptr = M === nothing ? C_NULL : handle(_base(M)).ptr
    _check(ccall((:bsm_bicgstab_create, libbsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Int32, Ref{Ptr{Cvoid}}),
        handle(_base(A)).ptr, _op(A), mptr, M === nothing ? 0 : _op(M), _DTYPE[T], k, out))
    p = BsmCgParams(sizeof(BsmCgParams), x0, rtol, atol, maxiter, maxiter)
    info = BsmCgInfo(0, 0, 0, 0, 0, 0, 0)
    columns = Vector{BsmCgColumn}(undef, k)
    history = zeros(Float64, k, max(maxiter, 1))
    ld = max(n, 1)
    try
        GC.@preserve A M X B columns history _check(ccall((:bsm_bicgstab_solve, libbsm), Cint,
            (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ref{BsmCgParams}, Ref{BsmCgInfo}, Ptr{BsmCgColumn}, Ptr{Float64}, Cint, Ptr{Cvoid}),
            out[], k, pointer(B), ld, pointer(X), ld, p, info, columns, history, 0, C_NULL))
    finally
        ccall((:bsm_bicgstab_destroy, libbsm), Cint, (Ptr{Cvoid},), out[])
    end
    return X, info, columns, history[:, 1:min(info.iterations, maxiter)]
end

"""
    minres!(X, A, B; M=nothing, rtol=1e-8, atol=0.0, maxiter=size(A, 1), x0=false) -> (X, info, columns, history)

Symmetric-preconditioned MINRES for `A X = B` with `A` real symmetric or Hermitian and not necessarily definite, and 1 to
16 right-hand sides advancing in lockstep on one multi-column product per iteration, every step of it on the device
(bsm_minres_create / _solve / _destroy).  The caller asserts the symmetry of `A` and that `M` is symmetric / Hermitian
positive definite.  `B` and `X` are host vectors or matrices of `A`'s element type, or complex ones of its precision under
real `A` and `M`.  Column `c` is converged when the 2-norm of its carried residual `b - A x` is
`<= max(rtol * norm(B[:, c]), atol)`.  `info`, `columns` and `history` are those of [`cg!`](@ref): `columns[c].status` 0
converged, 1 `maxiter` reached, 2 a non-finite residual, 3 breakdown (an indefinite `M`, a singular `A`);
`info.a_products == info.iterations`.  (The reference offers nothing here: a `LinearMap` is handed to a Julia solver
package, whose Krylov loop runs on the host.)
"""
function minres!(X::VecOrMat{T}, A::ROCmAnyOp, B::VecOrMat{T}; M=nothing, rtol::Real=1e-8, atol::Real=0.0,
                 maxiter::Integer=size(A, 1), x0::Bool=false) where {T<:ROCmEltype}
    n, k = size(B, 1), size(B, 2)
    size(A, 1) == size(A, 2) == n && size(X) == size(B) || throw(DimensionMismatch("minres! needs a square operator and B, X of its order"))
    1 <= k <= 16 || throw(ArgumentError("minres! takes 1 to 16 right-hand sides"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    mptr = M === nothing ? C_NULL : handle(_base(M)).ptr
    _check(ccall((:bsm_minres_create, libbsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Int32, Ref{Ptr{Cvoid}}),
        handle(_base(A)).ptr, _op(A), mptr, M === nothing ? 0 : _op(M), _DTYPE[T], k, out))
    p = BsmCgParams(sizeof(BsmCgParams), x0, rtol, atol, maxiter, maxiter)
    info = BsmCgInfo(0, 0, 0, 0, 0, 0, 0)
    columns = Vector{BsmCgColumn}(undef, k)
    history = zeros(Float64, k, max(maxiter, 1))
    ld = max(n, 1)
    try
        GC.@preserve A M X B columns history _check(ccall((:bsm_minres_solve, libbsm), Cint,
            (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ref{BsmCgParams}, Ref{BsmCgInfo}, Ptr{BsmCgColumn}, Ptr{Float64}, Cint, Ptr{Cvoid}),
            out[], k, pointer(B), ld, pointer(X), ld, p, info, columns, history, 0, C_NULL))
    finally
        ccall((:bsm_minres_destroy, libbsm), Cint, (Ptr{Cvoid},), out[])
    end
    return X, info, columns, history[:, 1:min(info.iterations, maxiter)]
end

"""
    lsqr!(X, A, B; rtol=1e-8, atol=0.0, ntol=1e-8, damp=0.0, maxiter=min(size(A)...), x0=false)
        -> (X, info, columns, history, normal_residual, anorm)

LSQR for `min ||B - A X||^2 + damp^2 ||X - X0||^2` with `A` of any shape and rank -- over-determined, under-determined (the
minimum-norm solution) or singular --, and 1 to 16 right-hand sides advancing in lockstep on two multi-column products per
iteration, one with `A` and one with `A'`, every step of it on the device (bsm_lsqr_create / _solve / _destroy).  `B` has
`size(A, 1)` rows, `X` `size(A, 2)`; both are host vectors or matrices of `A`'s element type, or complex ones of its
precision under a real `A`.  `transpose(A)` of a complex `A` is refused (its adjoint is `conj(A)`).  Column `c` stops with
status 0 when the estimate of `norm(b - A x)` is `<= max(rtol * norm(B[:, c]), atol)`, when the estimate of the
normal-equation residual is `<= ntol * anorm * ` that estimate, or when the Krylov space ends; 1 `maxiter` reached, 2 a
non-finite estimate.  `info`, `columns` and `history` are those of [`cg!`](@ref); `normal_residual` and `anorm` hold the two
estimates per column; `info.a_products == 2 * info.iterations + 1` (`+ 1` with `x0`).  There is no preconditioner argument.
(The reference offers nothing here: a `LinearMap` is handed to a Julia solver package, whose Krylov loop runs on the host.)
"""
function lsqr!(X::VecOrMat{T}, A::ROCmAnyOp, B::VecOrMat{T}; rtol::Real=1e-8, atol::Real=0.0, ntol::Real=1e-8, damp::Real=0.0,
               maxiter::Integer=min(size(A, 1), size(A, 2)), x0::Bool=false) where {T<:ROCmEltype}
    m, n, k = size(A, 1), size(A, 2), size(B, 2)
    size(B, 1) == m && size(X, 1) == n && size(X, 2) == k || throw(DimensionMismatch("lsqr! needs B with size(A, 1) rows and X with size(A, 2) rows and the columns of B"))
    1 <= k <= 16 || throw(ArgumentError("lsqr! takes 1 to 16 right-hand sides"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:bsm_lsqr_create, libbsm), Cint, (Ptr{Cvoid}, Cint, Cint, Int32, Ref{Ptr{Cvoid}}),
        handle(_base(A)).ptr, _op(A), _DTYPE[T], k, out))
    p = BsmLsqrParams(sizeof(BsmLsqrParams), x0, rtol, atol, ntol, damp, maxiter, maxiter)
    info = BsmCgInfo(0, 0, 0, 0, 0, 0, 0)
    columns = Vector{BsmCgColumn}(undef, k)
    history = zeros(Float64, k, max(maxiter, 1))
    normal_residual, anorm = zeros(Float64, k), zeros(Float64, k)
    try
        GC.@preserve A X B columns history normal_residual anorm _check(ccall((:bsm_lsqr_solve, libbsm), Cint,
            (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ref{BsmLsqrParams}, Ref{BsmCgInfo}, Ptr{BsmCgColumn}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Cint, Ptr{Cvoid}),
            out[], k, pointer(B), max(m, 1), pointer(X), max(n, 1), p, info, columns, history, normal_residual, anorm, 0, C_NULL))
    finally
        ccall((:bsm_lsqr_destroy, libbsm), Cint, (Ptr{Cvoid},), out[])
    end
    return X, info, columns, history[:, 1:min(info.iterations, maxiter)], normal_residual, anorm
end

# ---- extreme eigenpairs of symmetric / Hermitian operators (bsm_eigsh_*) and the basis compression (bsm_krylov_combine) ----
mutable struct BsmEigshParams       # mirrors bsm_eigsh_params (32 bytes)
    struct_size::Int32; which::Int32; rtol::Float64; atol::Float64; maxcycles::Int32; vectors::Int32
end
mutable struct BsmEigshInfo         # mirrors bsm_eigsh_info (48 bytes)
    status::Int32; nconv::Int32; cycles::Int32; reserved::Int32
    a_products::Int64; anorm::Float64; workspace_bytes::Int64; workspace::UInt64
end
struct BsmEigshPair                 # mirrors bsm_eigsh_pair (24 bytes)
    value::Float64; estimate::Float64; residual::Float64
end
const _EIGSH_WHICH = Dict(:LA => 0, :SA => 1, :BE => 2, :LM => 3)

"""
    eigsh!(X, A, v0; which=:LA, ncv=min(size(A, 1), 128, max(2 nev + 1, 20)), rtol=1e-10, atol=0.0, maxcycles=300, vectors=true)
        -> (w, X, info, pairs)

`nev = size(X, 2)` extreme eigenpairs of a real symmetric / Hermitian `A` by thick-restart Lanczos (the Hermitian
Krylov-Schur method that KrylovKit's `eigsolve` runs), the basis, the products, the orthogonalisation and the restart on the
device (bsm_eigsh_create / _solve / _destroy).  The caller asserts the symmetry.  `which`: `:LA` largest algebraic, `:SA`
smallest, `:BE` both ends (`cld(nev, 2)` from the top, the rest from the bottom), `:LM` largest magnitude.  `v0` (the start
vector) and `X` are host arrays of `A`'s element type; `nev + 2 <= ncv <= min(size(A, 1), 128)`.  Converged when every wanted
pair's estimate `|beta_m S[m, i]|` is `<= max(rtol * anorm, atol)`, `anorm` being the largest `|theta|` seen.  `info.status`:
0 converged, 1 `maxcycles` reached, 2 a non-finite norm or Ritz value, 3 the Krylov space ended before `nev` pairs existed.
`w` holds the `info.nconv` eigenvalues in the order of `which`, `X[:, 1:nconv]` their orthonormal vectors, `pairs[i]` value,
estimate and true residual.  Not in it: interior eigenvalues, shift-invert, the generalised problem, preconditioning,
multiplicities, singular values, block methods.
"""
function eigsh!(X::Matrix{T}, A::ROCmAnyOp, v0::Vector{T}; which::Symbol=:LA,
                ncv::Integer=min(size(A, 1), 128, max(2 * size(X, 2) + 1, 20)), rtol::Real=1e-10, atol::Real=0.0,
                maxcycles::Integer=300, vectors::Bool=true) where {T<:ROCmEltype}
    n, nev = size(X, 1), size(X, 2)
    size(A, 1) == size(A, 2) == n == length(v0) || throw(DimensionMismatch("eigsh! needs a square operator and v0, X of its order"))
    haskey(_EIGSH_WHICH, which) || throw(ArgumentError("which must be :LA, :SA, :BE or :LM"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:bsm_eigsh_create, libbsm), Cint, (Ptr{Cvoid}, Cint, Cint, Int32, Int32, Ref{Ptr{Cvoid}}),
        handle(_base(A)).ptr, _op(A), _DTYPE[T], nev, ncv, out))
    p = BsmEigshParams(sizeof(BsmEigshParams), _EIGSH_WHICH[which], rtol, atol, maxcycles, vectors)
    info = BsmEigshInfo(0, 0, 0, 0, 0, 0.0, 0, 0)
    pairs = Vector{BsmEigshPair}(undef, nev)
    try
        GC.@preserve A X v0 pairs _check(ccall((:bsm_eigsh_solve, libbsm), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ref{BsmEigshParams}, Ref{BsmEigshInfo}, Ptr{BsmEigshPair}, Cint, Ptr{Cvoid}),
            out[], pointer(v0), pointer(X), max(n, 1), p, info, pairs, 0, C_NULL))
    finally
        ccall((:bsm_eigsh_destroy, libbsm), Cint, (Ptr{Cvoid},), out[])
    end
    return [pairs[i].value for i in 1:info.nconv], X, info, pairs[1:info.nconv]
end

# ---- largest / smallest singular triplets of rectangular operators (bsm_svds_*) ----
mutable struct BsmSvdsParams        # mirrors bsm_svds_params (32 bytes)
    struct_size::Int32; which::Int32; rtol::Float64; atol::Float64; maxcycles::Int32; vectors::Int32
end
mutable struct BsmSvdsInfo          # mirrors bsm_svds_info (48 bytes)
    status::Int32; nconv::Int32; cycles::Int32; reserved::Int32
    a_products::Int64; anorm::Float64; workspace_bytes::Int64; workspace::UInt64
end
struct BsmSvdsTriplet               # mirrors bsm_svds_triplet (32 bytes)
    value::Float64; estimate::Float64; residual_av::Float64; residual_ahu::Float64
end
const _SVDS_WHICH = Dict(:LM => 0, :SM => 1)

"""
    svds!(U, V, A, v0; which=:LM, ncv=min(size(A)..., 128, max(2 nsv + 1, 20)), rtol=1e-10, atol=0.0, maxcycles=300, vectors=true)
        -> (s, U, V, info, triplets)

`nsv = size(U, 2)` largest (`:LM`) or smallest (`:SM`) singular triplets of a rectangular or nonsymmetric `A` (`m x n`) by
thick-restart Golub-Kahan-Lanczos bidiagonalisation with full two-sided reorthogonalisation (what KrylovKit's `svdsolve`
runs), the bases, both products, the orthogonalisation, the restart and the true residuals on the device (bsm_svds_create /
_solve / _destroy).  `U` (`m x nsv`), `V` (`n x nsv`) and `v0` (`min(m, n)` entries: the recurrence starts in the short space)
are host arrays of `A`'s element type; `nsv + 2 <= ncv <= min(m, n, 128)`.  `transpose(A)` of a complex `A` is refused (it
would need `conj(A)`).  Converged when every wanted triplet's estimate `|beta_m X[m, i]|` is `<= max(rtol * anorm, atol)`,
`anorm` being the largest `sigma` seen.  `info.status`: 0 converged, 1 `maxcycles` reached, 2 a non-finite norm or value or
the sweep cap of the small SVD, 3 the space ended before `nsv` triplets existed.  `s` holds the `info.nconv` values in the
order of `which`, `U[:, 1:nconv]`, `V[:, 1:nconv]` their orthonormal vectors, `triplets[i]` value, estimate and the true
residuals `||A v - sigma u||`, `||A' u - sigma v||`.  One product per step is a transposed one: two runs give the same bits only
on handles whose transposed product is reproducible (`transpose_image`).  NOT in it: one-sided reorthogonalisation, harmonic /
refined Ritz values or shift-invert for interior and tiny values, a block method, multi-device and own-range handles, graph
capture.
"""
function svds!(U::Matrix{T}, V::Matrix{T}, A::ROCmAnyOp, v0::Vector{T}; which::Symbol=:LM,
               ncv::Integer=min(size(A, 1), size(A, 2), 128, max(2 * size(U, 2) + 1, 20)), rtol::Real=1e-10, atol::Real=0.0,
               maxcycles::Integer=300, vectors::Bool=true) where {T<:ROCmEltype}
    m, n, nsv = size(A, 1), size(A, 2), size(U, 2)
    (size(U, 1) == m && size(V, 1) == n && size(V, 2) == nsv && length(v0) == min(m, n)) ||
        throw(DimensionMismatch("svds! needs U (m x nsv), V (n x nsv) and v0 of min(m, n) entries"))
    haskey(_SVDS_WHICH, which) || throw(ArgumentError("which must be :LM or :SM"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    _check(ccall((:bsm_svds_create, libbsm), Cint, (Ptr{Cvoid}, Cint, Cint, Int32, Int32, Ref{Ptr{Cvoid}}),
        handle(_base(A)).ptr, _op(A), _DTYPE[T], nsv, ncv, out))
    p = BsmSvdsParams(sizeof(BsmSvdsParams), _SVDS_WHICH[which], rtol, atol, maxcycles, vectors)
    info = BsmSvdsInfo(0, 0, 0, 0, 0, 0.0, 0, 0)
    triplets = Vector{BsmSvdsTriplet}(undef, nsv)
    try
        GC.@preserve A U V v0 triplets _check(ccall((:bsm_svds_solve, libbsm), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ref{BsmSvdsParams}, Ref{BsmSvdsInfo}, Ptr{BsmSvdsTriplet}, Cint,
             Ptr{Cvoid}),
            out[], pointer(v0), pointer(U), max(m, 1), pointer(V), max(n, 1), p, info, triplets, 0, C_NULL))
    finally
        ccall((:bsm_svds_destroy, libbsm), Cint, (Ptr{Cvoid},), out[])
    end
    return [triplets[i].value for i in 1:info.nconv], U, V, info, triplets[1:info.nconv]
end

"""
    krylov_combine!(Out, V, S, T, n, m, k; ldv=max(n, 1), lds=m, ldo=max(n, 1), carry=-1, stream=C_NULL)

`Out[:, c] = sum_j V[:, j] S[j, c]` for `c <= k` on the device (bsm_krylov_combine), the sum over `j` ascending with one fma
per term; with `carry >= 0` (a 0-based column of `V`, at most `m`) that column is also copied behind them.  `Out`, `V`, `S`
are DEVICE pointers (e.g. of AMDGPU.jl arrays): `V` `n x m` of element type `T`, `S` `m x k` of `real(T)`, column-major.
`Out == V` with `ldo == ldv` works in place.  Enqueues on `stream`; synchronises nothing.  `krylov_combine_tile(T, m)` is the
number of rows one workgroup stages.
"""
function krylov_combine!(Out::Ptr{Cvoid}, V::Ptr{Cvoid}, S::Ptr{Cvoid}, ::Type{T}, n::Integer, m::Integer, k::Integer;
                         ldv::Integer=max(n, 1), lds::Integer=m, ldo::Integer=max(n, 1), carry::Integer=-1,
                         stream::Ptr{Cvoid}=C_NULL) where {T<:ROCmEltype}
    _check(ccall((:bsm_krylov_combine, libbsm), Cint,
        (Cint, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}),
        _DTYPE[T], n, m, k, V, ldv, S, lds, Out, ldo, carry, stream))
    return Out
end
krylov_combine_tile(::Type{T}, m::Integer) where {T<:ROCmEltype} =
    ccall((:bsm_krylov_combine_tile, libbsm), Int64, (Cint, Int64), _DTYPE[T], m)

# ---- LOBPCG (bsm_lobpcg_*) and the two tall-skinny products of a block method (bsm_block_gram, bsm_block_combine) --------
mutable struct BsmLobpcgParams      # mirrors bsm_lobpcg_params (32 bytes)
    struct_size::Int32; which::Int32; rtol::Float64; atol::Float64; maxiter::Int32; reserved::Int32
end
mutable struct BsmLobpcgInfo        # mirrors bsm_lobpcg_info (48 bytes)
    status::Int32; nconv::Int32; iterations::Int32; drops::Int32
    a_products::Int64; m_products::Int64; anorm::Float64; workspace_bytes::Int64
end

"""
    lobpcg!(X, A, X0; M=nothing, which=:SA, rtol=1e-10, atol=0.0, maxiter=200) -> (w, X, info, pairs, history)

The `nev = size(X, 2)` smallest (`:SA`) or largest (`:LA`) eigenpairs of a real symmetric / Hermitian `A` by LOBPCG on the
block `X0` (`size(A, 1) x block`, `nev <= block <= 16`, `3 block <= size(A, 1)`), with an optional preconditioner `M` --
Hermitian positive definite, `~ inv(A)` on the wanted end: a block-Jacobi or a polynomial handle --, on the device
(bsm_lobpcg_create / _solve / _destroy).  The caller asserts both.  A block method finds every copy of a multiple eigenvalue;
`A` is streamed once per iteration for the whole block.  `X0` and `X` are host matrices of `A`'s element type.  Converged when
the carried residual norms of the first `nev` columns are `<= max(rtol * anorm, atol)`.  `info.status`: 0 converged, 1
`maxiter` reached, 2 a non-finite norm, Gram entry or Ritz value, 3 fewer than `block` directions kept (a rank-deficient
`X0`).  `w` holds the eigenvalues in the order of `which`, `pairs[i]` value, carried and true residual, `history` the carried
norms as `nev x (iterations + 1)`.  Per iteration the host synchronises once and runs a Rayleigh-Ritz step of order up to
`3 block`.
"""
function lobpcg!(X::Matrix{T}, A::ROCmAnyOp, X0::Matrix{T}; M=nothing, which::Symbol=:SA, rtol::Real=1e-10, atol::Real=0.0,
                 maxiter::Integer=200) where {T<:ROCmEltype}
    n, nev, block = size(X, 1), size(X, 2), size(X0, 2)
    size(A, 1) == size(A, 2) == n == size(X0, 1) || throw(DimensionMismatch("lobpcg! needs a square operator and X0, X of its order"))
    which in (:SA, :LA) || throw(ArgumentError("which must be :SA or :LA"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    mptr = M === nothing ? C_NULL : handle(_base(M)).ptr
    _check(ccall((:bsm_lobpcg_create, libbsm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Int32, Int32, Ref{Ptr{Cvoid}}),
        handle(_base(A)).ptr, _op(A), mptr, M === nothing ? 0 : _op(M), _DTYPE[T], nev, block, out))
    p = BsmLobpcgParams(sizeof(BsmLobpcgParams), _EIGSH_WHICH[which], rtol, atol, maxiter, 0)
    info = BsmLobpcgInfo(0, 0, 0, 0, 0, 0, 0.0, 0)
    pairs = Vector{BsmEigshPair}(undef, nev)
    history = fill(NaN, nev, maxiter + 1)
    try
        GC.@preserve A M X X0 pairs history _check(ccall((:bsm_lobpcg_solve, libbsm), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ref{BsmLobpcgParams}, Ref{BsmLobpcgInfo}, Ptr{BsmEigshPair}, Ptr{Float64}, Int64, Cint, Ptr{Cvoid}),
            out[], pointer(X0), max(n, 1), pointer(X), max(n, 1), p, info, pairs, history, maxiter + 1, 0, C_NULL))
    finally
        ccall((:bsm_lobpcg_destroy, libbsm), Cint, (Ptr{Cvoid},), out[])
    end
    return [pairs[i].value for i in 1:nev], X, info, pairs, history[:, 1:(info.status <= 1 ? info.iterations + 1 : 0)]
end

"""
    block_gram!(G, U, W, work, T, n, p, q; ldu=max(n, 1), ldw=max(n, 1), ldg=p, stream=C_NULL)

`G = U' W` on the device (bsm_block_gram): `U` `n x p` (`p <= 48`), `W` `n x q` (`q <= 96`) of element type `T`, `G` `p x q` of
the WIDE type (`Float64` / `ComplexF64`), `work` `block_gram_work(T, n, p, q)` bytes, 16-byte aligned; all DEVICE pointers,
column-major.  `W` may alias or contain `U`.  Partial sums per row range on the matrix pipe in the precision of `T`, added in a
fixed order in double.  Enqueues on `stream`; synchronises nothing.  `block_gram_grid(T, n)` is the number of row ranges.
"""
function block_gram!(G::Ptr{Cvoid}, U::Ptr{Cvoid}, W::Ptr{Cvoid}, work::Ptr{Cvoid}, ::Type{T}, n::Integer, p::Integer, q::Integer;
                     ldu::Integer=max(n, 1), ldw::Integer=max(n, 1), ldg::Integer=p, stream::Ptr{Cvoid}=C_NULL) where {T<:ROCmEltype}
    _check(ccall((:bsm_block_gram, libbsm), Cint,
        (Cint, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}),
        _DTYPE[T], n, p, U, ldu, q, W, ldw, G, ldg, work, stream))
    return G
end
block_gram_grid(::Type{T}, n::Integer) where {T<:ROCmEltype} = ccall((:bsm_block_gram_grid, libbsm), Int64, (Cint, Int64), _DTYPE[T], n)
block_gram_work(::Type{T}, n::Integer, p::Integer, q::Integer) where {T<:ROCmEltype} =
    ccall((:bsm_block_gram_work, libbsm), Int64, (Cint, Int64, Int64, Int64), _DTYPE[T], n, p, q)

"""
    block_combine!(Out, V, C, T, n, p, q; ldv=max(n, 1), ldc=p, ldo=max(n, 1), stream=C_NULL)

`Out[:, c] = sum_j V[:, j] C[j, c]` for `c <= q` on the device (bsm_block_combine) with `C` of element type `T` itself --
complex for complex `T` --, the sum over `j` ascending with fused multiply-adds.  `Out`, `V`, `C` are DEVICE pointers: `V`
`n x p` (`p <= 48`), `C` `p x q` (`q <= p`), column-major.  `Out == V` with `ldo == ldv` works in place.  Enqueues on `stream`;
synchronises nothing.  `block_combine_tile(T, p)` is the number of rows one workgroup stages.
"""
function block_combine!(Out::Ptr{Cvoid}, V::Ptr{Cvoid}, C::Ptr{Cvoid}, ::Type{T}, n::Integer, p::Integer, q::Integer;
                        ldv::Integer=max(n, 1), ldc::Integer=p, ldo::Integer=max(n, 1), stream::Ptr{Cvoid}=C_NULL) where {T<:ROCmEltype}
    _check(ccall((:bsm_block_combine, libbsm), Cint,
        (Cint, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
        _DTYPE[T], n, p, q, V, ldv, C, ldc, Out, ldo, stream))
    return Out
end
block_combine_tile(::Type{T}, p::Integer) where {T<:ROCmEltype} =
    ccall((:bsm_block_combine_tile, libbsm), Int64, (Cint, Int64), _DTYPE[T], p)

# ---- polynomial preconditioners as handles (bsm_poly_*) -----------------------------------------------------------------
"""
    PolynomialPreconditioner

`z = p(A) x` as a handle of its own (bsm_poly_create): `steps` steps of the recurrence `r_0 = x`, `d_0 = b_0 D r_0`,
`r_{k+1} = r_k - A d_k`, `d_{k+1} = a_{k+1} d_k + b_{k+1} D r_{k+1}`, `p(A) x = d_0 + ... + d_{steps-1}` with real
coefficients over an operator `A` and an optional inner preconditioner `D` (`nothing`: the identity).  Pass it as `M` to
`cg!`, `minres!`, `bicgstab!` and `gmres!`; it keeps `A` and `D` alive.  Its own product takes device vectors only, so
`mul!` with host arrays is not offered for it.  Built by `chebyshev_preconditioner` and `neumann_preconditioner`.
(The reference offers nothing here: a `LinearMap` is handed to a Julia solver package.)
"""
struct PolynomialPreconditioner
    handle::Handle
    source::Any
    inner::Any
    a::Vector{Float64}
    b::Vector{Float64}
end
handle(P::PolynomialPreconditioner) = P.handle
_base(P::PolynomialPreconditioner) = P
_op(::PolynomialPreconditioner) = 0
Base.size(P::PolynomialPreconditioner) = size(P.source)

function _polynomial(A::ROCmAnyOp, D, a::Vector{Float64}, b::Vector{Float64}, nrhs::Integer, ::Type{T}) where {T<:ROCmEltype}
    length(a) == length(b) && 1 <= length(b) <= 64 || throw(ArgumentError("a and b must have the same length, 1 to 64 steps"))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    dptr = D === nothing ? C_NULL : handle(_base(D)).ptr
    GC.@preserve A D a b _check(ccall((:bsm_poly_create, libbsm), Cint,
        (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cint, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ref{Ptr{Cvoid}}),
        handle(_base(A)).ptr, _op(A), dptr, D === nothing ? 0 : _op(D), _DTYPE[T], nrhs, length(b), a, b, out))
    return PolynomialPreconditioner(Handle(out[]), A, D, a, b)
end

"""
    polynomial_info(P) -> (steps, a, b, workspace_bytes)

What the library holds of a `PolynomialPreconditioner` (bsm_poly_info).
"""
function polynomial_info(P::PolynomialPreconditioner)
    steps, ws = Ref{Int32}(0), Ref{Int64}(0)
    a, b = zeros(Float64, 64), zeros(Float64, 64)
    _check(ccall((:bsm_poly_info, libbsm), Cint, (Ptr{Cvoid}, Ref{Int32}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}),
        P.handle.ptr, steps, a, b, ws))
    return Int(steps[]), a[1:steps[]], b[1:steps[]], ws[]
end

"""
    chebyshev_preconditioner(A, lmin, lmax, steps; D=nothing, nrhs=16, eltype=eltype(A))

The Chebyshev polynomial preconditioner of `steps` steps for a spectrum of `D A` inside `[lmin, lmax]`, `0 < lmin < lmax`
(Saad, Iterative Methods for Sparse Linear Systems, Alg. 12.1): `theta = (lmax + lmin) / 2`, `delta = (lmax - lmin) / 2`,
`sigma = theta / delta`, `rho_0 = 1 / sigma`, `b_0 = 1 / theta`, `rho_{k+1} = 1 / (2 sigma - rho_k)`,
`a_{k+1} = rho_{k+1} rho_k`, `b_{k+1} = 2 rho_{k+1} / delta`.  For symmetric / Hermitian positive definite `A` and `D`
(e.g. `block_jacobi(A, sets)`); `steps = 1` is `D / theta`.  Ritz values lie inside the spectrum: widen bounds taken from
a Lanczos run before use.
"""
function chebyshev_preconditioner(A::ROCmAnyOp, lmin::Real, lmax::Real, steps::Integer; D=nothing, nrhs::Integer=16, eltype::Type=Base.eltype(A))
    0 < lmin < lmax && isfinite(lmax) && steps >= 1 || throw(ArgumentError("chebyshev_preconditioner needs 0 < lmin < lmax and steps >= 1"))
    theta, delta = (Float64(lmax) + Float64(lmin)) / 2, (Float64(lmax) - Float64(lmin)) / 2
    sigma = theta / delta
    a, b = zeros(Float64, steps), zeros(Float64, steps)
    rho = 1 / sigma
    b[1] = 1 / theta
    for k in 2:steps
        nxt = 1 / (2 * sigma - rho)
        a[k], b[k] = nxt * rho, 2 * nxt / delta
        rho = nxt
    end
    return _polynomial(A, D, a, b, nrhs, eltype)
end

"""
    neumann_preconditioner(A, omega, steps; D=nothing, nrhs=16, eltype=eltype(A))

The Neumann (Richardson) polynomial preconditioner `omega sum_{k < steps} (I - omega D A)^k D`: `a_k = 0`, `b_k = omega`.
It approaches `inv(A)` as `steps` grows iff `rho(I - omega D A) < 1`; `A` need not be symmetric.
"""
function neumann_preconditioner(A::ROCmAnyOp, omega::Real, steps::Integer; D=nothing, nrhs::Integer=16, eltype::Type=Base.eltype(A))
    steps >= 1 && isfinite(omega) || throw(ArgumentError("neumann_preconditioner needs steps >= 1 and a finite omega"))
    return _polynomial(A, D, zeros(Float64, steps), fill(Float64(omega), steps), nrhs, eltype)
end

end # module
