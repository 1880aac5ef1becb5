!=======================================================================
! Shortwave radiation, shortwave = 'dEdd' (the delta-Eddington scheme), on the GPU for a caller of the reference's
! ice_shortwave and ice_step_mod.
!
! A module of its own name, next to ice_radiation_gpu (the ccsm3 scheme).  It offers
!   shortwave_dEdd            with the reference's interface (source/ice_shortwave.F90:1372-1386), forwarding to the
!                             block-wise entry cice_shortwave_dEdd of the GPU library (include/cice4_amd.h) through
!                             cice4_amd_c;
!   step_radiation_dedd_gpu   everything step_radiation does in its dEdd branch (source/ice_step_mod.F90:807-944) as the
!                             reference's own compute_coszen per block -- the orbital code stays on the host -- and ONE
!                             cice_step_radiation_dedd on the module arrays of ice_shortwave, ice_state and ice_flux.
! It is NOT a drop-in ice_shortwave: that module also owns the namelist's parameters (R_ice, R_pnd, R_snw are read from
! it), the category albedo arrays and init_shortwave, which stay where they are -- a caller writes
! `use ice_radiation_dedd_gpu, only: shortwave_dEdd` next to its `use ice_shortwave` of the rest.  The module holds no
! arithmetic of the scheme.
! cice_thermo_init and cice_shortwave_dedd_init are made on the first call, which is after the namelist.  The results stay
! on the device as after step_radiation_gpu: ice_radiation_gpu's prep_radiation_gpu does not know of this module and
! uploads the five arrays (sw_resident = 0), which gives the same bits.
!=======================================================================
      module ice_radiation_dedd_gpu

      use ice_kinds_mod
      use ice_domain_size, only: ncat, nilyr, nslyr, max_ntrcr
      use ice_constants
      use iso_c_binding
      use cice4_amd_c

      implicit none
      save
      private
      public :: shortwave_dEdd, step_radiation_dedd_gpu

      logical, private :: dedd_ready = .false., batch_ready = .false.

      contains

!=======================================================================
      subroutine dedd_ensure
      use ice_state, only: nt_Tsfc, nt_iage
      use ice_age, only: tr_iage
      use ice_meltpond, only: tr_pond
      use ice_therm_vertical, only: heat_capacity, calc_Tsfc, conduct, ustar_min
      use ice_shortwave, only: R_ice, R_pnd, R_snw
      type (cice_thermo_config) :: tcfg
      type (cice_dedd_config) :: cfg
      real (kind=dbl_kind) :: sal(nilyr+1), tml(nilyr+1)
      if (dedd_ready) return
      call cice_gpu_ensure()
      call cice_gpu_check(cice_check_sizes(cice_gpu_ctx, ncat, nilyr, nslyr, max_ntrcr), 'ice_radiation_dedd_gpu')
      tcfg%heat_capacity = merge(1, 0, heat_capacity)
      tcfg%calc_Tsfc = merge(1, 0, calc_Tsfc)
      tcfg%conduct = merge(0, 1, trim(conduct) == 'MU71')
      tcfg%ustar_min = ustar_min
      tcfg%tr_iage = merge(1, 0, tr_iage)
      tcfg%nt_Tsfc = nt_Tsfc
      tcfg%nt_iage = nt_iage
      call cice_gpu_check(cice_thermo_init(cice_gpu_ctx, tcfg, sal, tml), 'cice_thermo_init')
      cfg%R_ice = R_ice
      cfg%R_pnd = R_pnd
      cfg%R_snw = R_snw
      cfg%awtvdr = awtvdr
      cfg%awtidr = awtidr
      cfg%awtvdf = awtvdf
      cfg%awtidf = awtidf
      cfg%tr_pond = merge(1, 0, tr_pond)
      call cice_gpu_check(cice_shortwave_dedd_init(cice_gpu_ctx, cfg), 'cice_shortwave_dedd_init')
      dedd_ready = .true.
      end subroutine dedd_ensure

!=======================================================================
      subroutine dedd_batch
      use ice_blocks, only: nx_block, ny_block
      use ice_domain, only: nblocks
      if (batch_ready) return
      call cice_gpu_check(cice_thermo_batch_alloc(cice_gpu_ctx, nx_block, ny_block, nblocks), 'ice_radiation_dedd_gpu')
      batch_ready = .true.
      end subroutine dedd_batch

!=======================================================================
      subroutine shortwave_dEdd  (nx_block, ny_block,    &
                                  icells,   indxi,       &
                                  indxj,    coszen,      &
                                  aice,     vice,        &
                                  vsno,     fs,          &
                                  rhosnw,   rsnw,        &
                                  fp,       hp,          &
                                  swvdr,    swvdf,       &
                                  swidr,    swidf,       &
                                  alvdr,    alvdf,       &
                                  alidr,    alidf,       &
                                  fswsfc,   fswint,      &
                                  fswthru,  Sswabs,      &
                                  Iswabs,   albice,      &
                                  albsno,   albpnd)
      integer (kind=int_kind), intent(in) :: nx_block, ny_block, icells
      integer (kind=int_kind), dimension (nx_block*ny_block), intent(in) :: indxi, indxj
      real (kind=dbl_kind), dimension (nx_block,ny_block), intent(in) :: &
         coszen, aice, vice, vsno, fs, fp, hp, swvdr, swvdf, swidr, swidf
      real (kind=dbl_kind), dimension (nx_block,ny_block,nslyr), intent(in) :: rhosnw, rsnw
      real (kind=dbl_kind), dimension (nx_block,ny_block), intent(out) :: &
         alvdr, alvdf, alidr, alidf, fswsfc, fswint, fswthru, albice, albsno, albpnd
      real (kind=dbl_kind), dimension (nx_block,ny_block,nslyr), intent(out) :: Sswabs
      real (kind=dbl_kind), dimension (nx_block,ny_block,nilyr), intent(out) :: Iswabs

      call dedd_ensure
      call cice_gpu_check(cice_shortwave_dEdd(cice_gpu_ctx, nx_block, ny_block, icells, indxi, indxj, coszen, aice, vice, &
         vsno, fs, rhosnw, rsnw, fp, hp, swvdr, swvdf, swidr, swidf, alvdr, alvdf, alidr, alidf, fswsfc, fswint, fswthru, &
         Sswabs, Iswabs, albice, albsno, albpnd), 'shortwave_dEdd')
      end subroutine shortwave_dEdd

!=======================================================================
! state_resident: the state is what cice_step_ridge (step_ridge_gpu) left on the device in this step
      subroutine step_radiation_dedd_gpu (dt, state_resident)
      use ice_blocks, only: nx_block, ny_block
      use ice_domain, only: nblocks
      use ice_grid, only: tmask, tlat, tlon
      use ice_orbital, only: compute_coszen
      use ice_meltpond, only: tr_pond
      use ice_therm_vertical, only: calc_Tsfc
      use ice_state, only: aicen, trcrn, vicen, vsnon, apondn, hpondn
      use ice_flux, only: swvdr, swvdf, swidr, swidf, coszen
      use ice_shortwave, only: alvdrn, alidrn, alvdfn, alidfn, albicen, albsnon, albpndn, fswsfcn, fswintn, fswthrun, &
                               Sswabsn, Iswabsn
      real (kind=dbl_kind), intent(in) :: dt
      logical (kind=log_kind), intent(in), optional :: state_resident
      type (cice_radiation_dedd_fields) :: f
      integer (kind=int_kind) :: i, j, iblk, icells
      integer (kind=int_kind), dimension (nx_block*ny_block) :: indxi, indxj

      call dedd_ensure
      call dedd_batch
      if (calc_Tsfc) then
         do iblk = 1, nblocks
            icells = 0                    ! ice-ocean cells, as step_radiation lists them (:825-834)
            do j = 1, ny_block
            do i = 1, nx_block
               if (tmask(i,j,iblk)) then
                  icells = icells + 1
                  indxi(icells) = i
                  indxj(icells) = j
               endif
            enddo
            enddo
            call compute_coszen (nx_block, ny_block, icells, indxi, indxj, tlat(:,:,iblk), tlon(:,:,iblk), &
                                 coszen(:,:,iblk), dt)
         enddo
      endif
      f%ncat = ncat
      f%state_resident = 0
      if (present(state_resident)) f%state_resident = merge(1, 0, state_resident)
      f%aicen = addr_r8(aicen); f%trcrn = addr_r8(trcrn); f%vicen = addr_r8(vicen); f%vsnon = addr_r8(vsnon)
      f%swvdr = addr_r8(swvdr); f%swvdf = addr_r8(swvdf); f%swidr = addr_r8(swidr); f%swidf = addr_r8(swidf)
      f%coszen = addr_r8(coszen)
      f%apondn = c_null_ptr
      f%hpondn = c_null_ptr
      if (tr_pond) then
         f%apondn = addr_r8(apondn)
         f%hpondn = addr_r8(hpondn)
      endif
      f%alvdrn = addr_r8(alvdrn); f%alidrn = addr_r8(alidrn); f%alvdfn = addr_r8(alvdfn); f%alidfn = addr_r8(alidfn)
      f%albicen = addr_r8(albicen); f%albsnon = addr_r8(albsnon); f%albpndn = addr_r8(albpndn)
      f%fswsfcn = addr_r8(fswsfcn); f%fswintn = addr_r8(fswintn); f%fswthrun = addr_r8(fswthrun)
      f%Sswabsn = addr_r8(Sswabsn); f%Iswabsn = addr_r8(Iswabsn)
      call cice_gpu_check(cice_step_radiation_dedd(cice_gpu_ctx, f), 'step_radiation_dedd_gpu')
      end subroutine step_radiation_dedd_gpu

      end module ice_radiation_dedd_gpu
